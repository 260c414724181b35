"""CPU: the table of tests/rollout_kernels.py reaches every cell of its coverage lists, every float32 restatement of a kernel's algorithm
stays inside the family's tau against the float64 reference on every row, every mutant of a restatement leaves the bound on the rows named
for it by MIN_MARGIN at the least (test_mutant_margins prints the margins with -s), and the restated launch geometry is the sources'.
The middle two anchor the error scales before any GPU run: a restatement of a correct algorithm that does not fit means the scale is
wrong, a mutant that fits means the row is too weak."""
import os
import re

import numpy as np
import pytest
import torch

import rollout_kernels as R
from elem_bound import TAU_FP32
from m2h import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNT = {"gae": 144, "adv": 15, "reward": 52, "step_stats": 15, "mem": 24, "glue": 45, "copy": 49}
MARGINS = {}


def _ids(family, pred=lambda r: True):
    return [r["id"] for r in R.ROWS[family] if pred(r)]


@pytest.mark.parametrize("family", sorted(R.ROWS))
def test_rows_reach_every_cell(family):
    reached = {}
    for row in R.ROWS[family]:
        for c in R.cells(row):
            reached.setdefault(c, []).append(row["id"])
    missing = R.all_cells(family) - set(reached)
    assert not missing, sorted(map(str, missing))
    assert not set(reached) - R.all_cells(family)
    for c in sorted(R.all_cells(family), key=str):
        print("%-70s %s" % (c, ", ".join(reached[c][:3])))
    assert len({r["id"] for r in R.ROWS[family]}) == len(R.ROWS[family]) == ROW_COUNT[family]      # (a row taken out fails here or above)


def test_the_rows_are_the_issues_table():
    assert {(r["T"], r["N"], r["gae"]) for r in R.GAE_ROWS} == {(T, N, g) for T in (1, 2, 9) for N in (1, 63, 64, 65) for g in (0, 1)}
    assert R.GAE_GT == {"g0.99t0.95": (0.99, 0.95), "g1t1": (1.0, 1.0), "g0.99t0": (0.99, 0.0)}
    assert {(r["gae"], r["gt"], r["mask"]) for r in R.GAE_ROWS} == {(g, t, m) for g in (0, 1) for t in R.GAE_GT for m in ("ones", "random", "ends", "zeros")}
    assert {(r["n"], r["dist"]) for r in R.ADV_ROWS} == {(n, d) for n in (2, 255, 256, 257, 4097) for d in ("std", "off100s1", "off100s0.01")}
    L = (1, 1023, 1024, 1025, 4096, 4097, 16384)
    assert {(r["L"], r["N"], r["off"]) for r in R.REWARD_ROWS if r["kernel"] == "sq_stats"} == {(l, n, o) for l in L for n in (1, 3) for o in (0, 2)}
    assert {(r["L"], r["nch"], r["mix"], r["Cp"], r["Cg"]) for r in R.REWARD_ROWS if r["kernel"] == "stft_l2"} == \
        {(l,) + v for l in L for v in ((1, False, 1, 4), (2, True, 2, 8))}
    assert {(r["N"], r["quality"], r["mult"]) for r in R.REWARD_ROWS if r["kernel"] == "rewards_from_stats"} == \
        {(n, q, m) for n in (1, 64, 65) for q, m in ((True, 10.0), (False, 10.0), (False, 20.0))}
    assert {(r["L"], r["oe"]) for r in R.STEP_ROWS} == {(l, o) for l in (1, 15, 17, 4097, 16384) for o in R.STEP_OE}
    assert {r["N"] for r in R.STEP_ROWS} == {1, 3, 14} and {r["A"] for r in R.STEP_ROWS} == {1, 3}
    assert {r["B"] for r in R.MEM_ROWS} == {1, 2, 15}
    assert {(r["nd"], r["w"], r["x"]) for r in R.MEM_ROWS if r["B"] == 2} == {(n, w, x) for n in R.MEM_ND for w in R.MEM_W for x in R.MEM_IN}
    big = [r for r in R.GLUE_ROWS if r["kernel"] == "slice_concat_input" and r["B"] > 3]
    assert len(big) == 1 and (big[0]["F"], big[0]["T"]) == (512, 32) and big[0]["B"] * (big[0]["Ca"] + big[0]["Cb"]) > 256
    # the only rows past a megabyte are the grid-stride rows
    for r in R.GLUE_ROWS:
        nbytes = 16 * R.glue_total(r)
        assert (nbytes > 2 ** 20) == R.enters_grid_stride_loop(R.glue_total(r), R.GLUE_CAP), r["id"]


def test_restated_launch_geometry_is_the_sources():
    src = lambda n: open(os.path.join(ROOT, "move2hear-active-av-separation_amd", "csrc", n)).read()      # noqa: E731
    hdr = open(os.path.join(ROOT, "include", "m2h.h")).read()
    assert int(re.search(r"#define M2H_STEP_STATS_CHUNKS (\d+)", hdr).group(1)) == R.STEP_STATS_CHUNKS == _lib.STEP_STATS_CHUNKS
    assert int(re.search(r"#define M2H_ROWS_COPY_MAX (\d+)", hdr).group(1)) == R.ROWS_COPY_MAX == _lib.ROWS_COPY_MAX
    adv, losses, fused, ops_, mem, common = (src(n) for n in ("advantage.hip", "losses.hip", "rollout_fused.hip", "rollout_ops.hip", "acoustic_mem.hip", "rl_common.h"))
    assert "M2H_LAUNCH(gae_returns_kernel, dim3((N + %d) / %d), dim3(%d)" % (R.GAE_BLOCK - 1, R.GAE_BLOCK, R.GAE_BLOCK) in adv
    for k in ("advantages_kernel", "adv_sqdiff_kernel"):
        assert "M2H_LAUNCH(%s, dim3(1), dim3(%d)" % (k, R.ADV_BLOCK) in adv
    assert "for (int i = threadIdx.x; i < n; i += %d)" % R.ADV_BLOCK in adv
    assert "M2H_LAUNCH(adv_apply_kernel, dim3((n + 255) / 256), dim3(256)" in adv
    for k in ("sq_stats_kernel", "stft_l2_kernel"):
        assert "M2H_LAUNCH(%s, dim3(N), dim3(%d)" % (k, R.REWARD_BLOCK) in losses
    assert losses.count("i0 += %d)" % (R.REWARD_BLOCK * R.REWARD_UNROLL)) == 2 and losses.count("const int i = i0 + %d * u;" % R.REWARD_BLOCK) == 2
    assert "M2H_LAUNCH(rewards_from_stats_kernel, dim3((N + 63) / 64), dim3(%d)" % R.REWARDS_BLOCK in losses
    assert "dim3(M2H_STEP_STATS_CHUNKS, a.N), dim3(%d)" % R.STEP_STATS_BLOCK in fused and "per = (L + CH - 1) / CH" in fused
    assert "for (int i = i0 + tid; i < i1; i += %d)" % R.STEP_STATS_BLOCK in fused
    assert "(big / 16 + 255) / 256 > %d ? %d" % (R.ROWS_COPY_GX, R.ROWS_COPY_GX) in ops_ and "gx > %d ? %d : gx" % (R.OBSERVE_GX, R.OBSERVE_GX) in ops_
    assert "((Lw & 3) ? Lw : Lw / 4), %d)" % R.GATHER_CAP in ops_
    assert "unsigned cap = %d" % R.GLUE_CAP in common and "dim3(grid_for(total)), dim3(256)" in ops_ and "dim3(grid_for(npix)), dim3(256)" in ops_
    assert "constexpr int MEM_R = %d;" % R.MEM_R in mem and "dim3(B * (32 / m2h::MEM_R)), dim3(256)" in mem
    # what the geometry means for the rows
    assert R.step_slices(1) == (1, 1) and R.step_slices(15) == (1, 15) and R.step_slices(17) == (2, 9) and R.step_slices(4097) == (257, 16)
    assert R.step_slices(16384) == (1024, 16)
    assert not R.enters_grid_stride_loop(R.GATHER_CAP * 256, R.GATHER_CAP) and R.enters_grid_stride_loop(R.gather_items(1, 699100, 3), R.GATHER_CAP)
    assert R.rows_copy_threads(1028, R.ROWS_COPY_GX) == 256 and R.rows_copy_threads(2 ** 21, R.ROWS_COPY_GX) == 65536
    assert R.rows_copy_threads(2 ** 21, R.OBSERVE_GX) == 16384
    assert R.rows_copy_second_pass(1028, 1028, R.ROWS_COPY_GX) and not R.rows_copy_second_pass(2 ** 20, 2 ** 20, R.ROWS_COPY_GX)
    assert R.rows_copy_second_pass(2 ** 20 + 16, 2 ** 20 + 16, R.ROWS_COPY_GX) and R.rows_copy_second_pass(262144 + 16, 262144 + 16, R.OBSERVE_GX)
    assert R.STATS_FIELDS == tuple(_lib.EPISODE_STATS_FIELDS)


def _within(family, row, got, ref, what="restatement"):
    worst_all = 0.0
    for name, rs in ref.items():
        if name == "near_clamp" or name not in got:
            continue
        r, s = rs
        g = np.asarray(got[name], dtype=np.float64)
        assert np.isfinite(g).all(), (row["id"], name)
        worst, scale, ok = R.check(g.reshape(np.shape(r)), r, s, R.TAU[family])
        assert ok, (what, row["id"], name, worst, scale)
        worst_all = max(worst_all, worst)
    assert any(n in got for n in ref), row["id"]
    return worst_all


def _margin(family, got, ref):
    """By how many tau the bound rejects `got` (its worst output): inf where an exact output differs or a value is not finite."""
    m = 0.0
    for name, rs in ref.items():
        if name == "near_clamp" or name not in got:
            continue
        r, s = rs
        g = np.asarray(got[name], dtype=np.float64)
        if not np.isfinite(g).all():
            return float("inf")
        worst = R.check(g.reshape(np.shape(r)), r, s, R.TAU[family])[0]
        m = max(m, worst / R.TAU[family]) if worst == worst else float("inf")
    return m


def _state(got):
    return {k: got[k] for k in ("mean", "mean1", "mean_b", "sqdiff_a", "sqdiff_b")}


def _mutants_of(family, row):
    return [m for m, (f, pred) in R.MUTANT_ROWS.items() if f == family and pred(row)]


def _restatement_and_mutants(family, row, inp=None):
    inp = R.inputs(row) if inp is None else inp
    got = R.FP32[family](row, inp)
    ref = R.reference(row, inp, _state(got) if family == "adv" else None)
    worst = _within(family, row, got, ref)
    for m in _mutants_of(family, row):
        mg = R.FP32[family](row, inp, m)
        mref = R.reference(row, inp, _state(mg)) if family == "adv" else ref
        margin = _margin(family, mg, mref)
        MARGINS[(family, m)] = min(MARGINS.get((family, m), float("inf")), margin)
        assert margin >= R.MIN_MARGIN, (row["id"], m, margin)
    return inp, got, ref, worst


def test_every_mutant_has_rows_and_every_family_keeps_tau_fp32():
    for m, (f, pred) in R.MUTANT_ROWS.items():
        assert sum(1 for r in R.ROWS[f] if pred(r)) >= 2, m
    assert set(R.MUTANT_ROWS) == set(R.GAE_MUTANTS + R.ADV_MUTANTS + R.REWARD_MUTANTS + R.STEP_MUTANTS + R.MEM_MUTANTS + R.GLUE_MUTANTS)
    assert all(R.TAU[f] == TAU_FP32 for f in R.FAMILIES)        # (a wider bound would need a restatement beyond TAU_FP32: the tests below find none)


@pytest.mark.parametrize("row_id", _ids("gae"))
def test_gae_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("gae", row)
    T = row["T"]
    if row["gae"]:          # what the scan must not write, and what it must
        assert (got["returns"][T] == R.GAE_SENTINEL).all() and (got["value_preds"][T] == inp["next_value"].numpy().reshape(-1)).all()
    else:
        assert (got["value_preds"] == inp["value_preds"].numpy().reshape(T + 1, -1)).all() and (got["returns"][T] == inp["next_value"].numpy().reshape(-1)).all()


@pytest.mark.parametrize("row_id", _ids("adv"))
def test_adv_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("adv", row)
    r, s = ref["mean"]
    ratio = abs(float(got["mean"]) - float(r)) / float(s)
    print("%s  mean ratio %.2e" % (row_id, ratio))
    if row["dist"] != "std":        # the rounding of a mean near 100 against sqrt(sum s(a)^2) / n grows with sqrt(n): why these rows stop at n = 4097
        assert ratio <= TAU_FP32 / 2, (row_id, ratio)
        one = R.adv_fp32(row, inp, R.ADV_MUTANTS[1])
        assert not R.check(one["var"], *R.reference(row, inp, _state(one))["var"], R.TAU["adv"])[2], row_id


@pytest.mark.parametrize("row_id", _ids("reward"))
def test_reward_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("reward", row)
    if row["kernel"] == "rewards_from_stats":
        done = inp["not_done"].numpy().reshape(-1) == 0
        assert (got["rewards"][done] == 0).all() and (ref["rewards"][1][done] == 0).all()
        if row["near"]:     # the reward is orders below the ratios it is the difference of: the scale, not an absolute tolerance, admits the float32 result
            r, s = ref["rewards"]
            assert float(np.abs(r[~done]).max()) < 1e-4 * float(s[~done].min())


@pytest.mark.parametrize("row_id", _ids("step_stats"))
def test_step_stats_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("step_stats", row)
    if R.STEP_OE[row["oe"]][0] == 0:
        assert (got["rewards"] == inp["env_rewards"].numpy().reshape(-1)).all()


def test_episode_bookkeeping_is_the_plain_float64_bookkeeping_rounded_once_per_operation():
    """episode_bookkeeping (the float32 judge of the fused kernel's statistics) against the same formulas in float64: they agree to float32
    rounding, finished envs reset their running sums, the others keep them."""
    row = R.ROWS_BY_ID[_ids("step_stats", lambda r: r["N"] == 14 and r["A"] == 3)[0]]
    inp = R.inputs(row)
    got = R.step_fp32(row, inp)
    r, losses = torch.from_numpy(got["rewards"]), torch.from_numpy(got["losses"])
    after = R.episode_bookkeeping(inp["stats"], r, losses, inp["probs"], inp["not_done"], inp["ndgs"], inp["dgs"])
    after64 = R.episode_bookkeeping({k: v.double() for k, v in inp["stats"].items()}, r.double(), losses.double(), inp["probs"].double(), inp["not_done"].double(),
                                    None if inp["ndgs"] is None else inp["ndgs"].double(), None if inp["dgs"] is None else inp["dgs"].double())
    assert set(after) == set(R.STATS_FIELDS)
    done = inp["not_done"].reshape(-1) == 0
    assert bool(done.any()) and not bool(done.all())
    for n in R.STATS_FIELDS:
        assert after[n].dtype == torch.float32 and torch.allclose(after[n], after64[n].float(), rtol=1e-6, atol=1e-6), n
    assert float(after["current_episode_step"][done].abs().sum()) == 0 and bool((after["current_episode_step"][~done] > 1).all())


@pytest.mark.parametrize("row_id", _ids("mem"))
def test_mem_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("mem", row)
    if row["w"] == "positive" and row["nd"] != "zero":
        F_ = torch.nn.functional
        nd = inp["not_done"]
        h0 = F_.conv2d(R.mem_sliced(inp["pred_mono"].double(), inp["prev_mem"].double(), nd.double() if nd is not None else None), inp["w0"].double(), None, 1, 1)
        assert float(h0.min()) >= 0.0 and float(h0.max()) > 0.0
    if row["nd"] == "zero":         # bit-identical to the output with a zero previous memory
        z = R.mem_fp32(row, dict(inp, prev_mem=torch.zeros_like(inp["prev_mem"])))
        assert np.array_equal(z["out"], got["out"]) and float(inp["prev_mem"].abs().sum()) > 0
    if row["B"] == 2:               # image b of the batch == the same image alone
        one = {k: (v[1:2] if k in ("pred_mono", "prev_mem") or (k == "not_done" and v is not None) else v) for k, v in inp.items()}
        assert np.array_equal(R.mem_fp32(dict(row, B=1), one)["out"][0], got["out"][1])


@pytest.mark.parametrize("row_id", _ids("mem", lambda r: r["B"] <= 2 and (r["x"] == "impulse" or r["w"] == "positive")))
def test_impulse_border_rows_and_positive_weight_rows_reject_the_halo_mutants(row_id):
    """The hidden rows outside the image, and each of the four halo columns: rejected on every impulse-border row and on every positive-weight
    row, and on the rows that are both through the border outputs alone (the rest of an impulse image's output is zero)."""
    row = R.ROWS_BY_ID[row_id]
    inp = R.inputs(row)
    ref = R.reference(row, inp)
    for m in R.MEM_MUTANTS[:5]:
        assert _margin("mem", R.mem_fp32(row, inp, m), ref) >= R.MIN_MARGIN, (row_id, m)
    if row["x"] == "impulse":
        r = ref["out"][0].reshape(row["B"], 16, 32, 32)
        assert float(np.abs(r[:, :, 3:29, :]).max()) == 0.0 and float(np.abs(r[:, :, :, 3:29]).max()) == 0.0 and float(np.abs(r).max()) > 0.0


@pytest.mark.parametrize("row_id", _ids("glue"))
def test_glue_restatement_fits_and_mutants_do_not(row_id):
    row = R.ROWS_BY_ID[row_id]
    inp, got, ref, _ = _restatement_and_mutants("glue", row)
    if row["kernel"] == "visual_input":
        assert np.array_equal(got["out"].astype(np.float64), ref["out"][0])
        return
    near = ref["near_clamp"]
    assert near.shape == ref["out"][0].shape
    if row["op"]:
        assert float(near.mean()) <= 0.01, (row_id, float(near.mean()))      # a condition on the inputs chosen, not a measurement
        assert bool((ref["out"][0] == 0).any()) and bool((ref["out"][0] > 0).any())       # the clamp acts
    else:
        assert not near.any()


def test_copy_rows_restate_to_plain_indexing():
    """The copy family's references are torch / numpy indexing; what is restated here is the pose update and the step counters."""
    for row in R.ROWS["copy"]:
        if row["kernel"] == "synth_env_step":
            inp = R.env_step_inputs(row)
            a, node, angle = (inp[k].numpy() for k in ("actions", "node", "angle"))
            n1, a1 = R.synth_env_step_reference(a, node, angle, row["n_nodes"])
            assert ((0 <= n1) & (n1 < row["n_nodes"]) & (0 <= a1) & (a1 < 4)).all()
            still = (a < 0) | (a > 2)
            assert (n1[still] == node[still]).all() and (a1[still] == angle[still]).all()
            if row["N"] >= 64:
                assert set(a.tolist()) == {-1, 0, 1, 2, 3} and bool(((a == 0) & (node == row["n_nodes"] - 1) & (n1 == 0)).any())
                assert bool(((a == 2) & (a1 < angle)).any()) and bool(((a == 1) & (a1 == 0) & (angle == 3)).any())
        if row["kernel"] == "step_index_advance":
            assert R.step_index_reference(row) == {"T1": (0, 1, 1), "wrap": (0, 1, 1), "mid": (2, 3, 3), "T_pol_ne_T_sep": (0, 1, 1)}[row["kind"]]


def test_zz_mutant_margins():
    """(summary: by how many tau each mutant leaves the bound, the least over its named rows; the module docstring of tests/rollout_kernels.py
    records them)"""
    for (family, m), v in sorted(MARGINS.items()):
        print("margin  %-10s %-70s %.1e" % (family, m, v))
    if len(MARGINS) == len(R.MUTANT_ROWS):      # (the whole file ran)
        assert min(MARGINS.values()) >= R.MIN_MARGIN
