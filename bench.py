#!/usr/bin/env python3
"""Headline benchmark: passive U-Net separator pair (get_binSepMasks + convert_bin2mono), spectrograms/s.

    python bench.py --gpus N --steps K --warmup W        (N > 1 without a launcher: this process starts the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path over one batch of synthetic 512xTm binaural log-magnitude spectrograms
already resident in HBM (BASELINE.json configs[1]: batch 256, 512x256).  The path shards by batch with no
data-path collective, so N ranks each run the full batch: weak scaling, value = all ranks'
spectrograms / max-over-ranks time.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line; everything else below runs only with --full:

    python bench.py --gpus 1 --steps K --warmup W --full

--dump-outputs DIR writes what the timed path returned in its last timed step (the two U-Nets' outputs; a fixed, seeded sample
of the batch when the whole would exceed 48 MiB) as DIR/<name>.npy in float32: the inputs and weights are seeded, so two builds
compare output for output.

Extra objects on the line (--full):
  roofline     dominant kernel family (the MFMA implicit-GEMM conv): algorithmic FLOP / HIP-event time,
               measured inside the timed region on the launch stream.
  cpu_baseline the oracle (oracle/m2h_oracle.py, a PyTorch-CPU restatement of the reference) timed on this
               host's cores on a bounded sample of the same workload (kind "port").
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "move2hear-active-av-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16X3_TFLOPS = 2500.0 / 3  # dense bf16 MFMA peak over the three products of a bf16x3 product
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tm", type=int, default=256, help="time frames (32 = reference-native, 256 = headline)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: per-kernel roofline pass, the other arithmetic modes and their parity, CPU baselines, the DD-PPO, "
                         "passive-training and feeder legs, clock probe (the options below shape those)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the timed path's outputs of its last timed step as DIR/<name>.npy (float32; seeded batch sample above 48 MiB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--feeder-steps", type=int, default=10, help="timed batches of the GPU audio feeder leg (0 = skip)")
    ap.add_argument("--feeder-batch", type=int, default=64)
    ap.add_argument("--no-far-target", action="store_true", help="skip the far-target / mixed-precision DD-PPO leg")
    ap.add_argument("--no-graph", action="store_true", help="enqueue the pair kernel by kernel instead of replaying a HIP graph")
    ap.add_argument("--ddppo-cycles", type=int, default=4, help="timed DD-PPO cycles (0 = skip); two untimed warm-up cycles precede them")
    ap.add_argument("--force-schedule", choices=["overlap", "buckets"], default=None, help="as --force-buckets, one half of it only (A/B)")
    ap.add_argument("--force-buckets", action="store_true",
                    help="DD-PPO legs at one rank: run the N > 1 gradient schedule anyway (two buckets, split backward as two HIP graphs, side-stream "
                         "steps; no collective at world size 1) -- what that schedule costs beside the one-rank one")
    ap.add_argument("--tail-overlap", action="store_true",
                    help="DD-PPO legs: enqueue the cycle's six update_sep on a second stream beside the last update_pol (overlap_update_tail; measured +0.5 %%: off)")
    ap.add_argument("--sep-update-math", choices=["fp32", "bf16x3"], default="bf16x3",
                    help="near-target DD-PPO leg: arithmetic of update_sep's launches (its convs over the 1680 stored samples are the cycle's one "
                         "matrix-bound phase); rollout and update_pol compute in fp32 either way")
    ap.add_argument("--math", choices=["fp32", "bf16x3"], default="bf16x3",
                    help="arithmetic of the conv engine in the timed U-Net pair: fp32 MFMA (exact products) or bf16x3 split products")
    ap.add_argument("--no-other-mode", action="store_true",
                    help="skip the pass in the other arithmetic (and the parity figure between the two): a profile of this run then holds the headline mode's kernels only")
    ap.add_argument("--train-steps", type=int, default=10, help="timed passive pre-training steps (0 = skip)")
    ap.add_argument("--train-math", choices=["fp32", "bf16x3"], default="fp32",
                    help="arithmetic of the forward / input-gradient GEMMs of the passive training leg (weight gradients, BatchNorm, Adam stay fp32)")
    ap.add_argument("--train-batch", type=int, default=64, help="pretrain_passive.yaml BATCH_SIZE")
    ap.add_argument("--train-tm", type=int, default=32, help="time frames of the training clips (32 = 1 s, the reference's)")
    ap.add_argument("--no-clock-probe", action="store_true",
                    help="skip the in-kernel clock probe (tools/clock_probe.py on the diagnostic library, a child process after the timed regions: roofline.clock_ghz)")
    ap.add_argument("--knobs", default="", help="A/B only: m2h_tuning_set pairs 'knob=value,...' (include/m2h_tuning.h: kernels that compute the same values)")
    return ap.parse_args()


def make_policy(dev, seed=1):
    from m2h import synthetic
    from m2h.common.spaces import move2hear_observation_space
    from m2h.pretrain.passive.policy import Move2HearPassiveWoMemoryPolicy
    pol = Move2HearPassiveWoMemoryPolicy(move2hear_observation_space())
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict(synthetic.passive_shapes(), seed).items()}
    pol.load_state_dict(sd)
    return pol.to(dev).eval(), sd


def make_inputs(dev, batch, tm, seed):
    """Seeded synthetic spectrograms generated on the device (same distribution as m2h.synthetic: log1p of a
    Rayleigh magnitude with a per-frequency gain); kept resident in HBM."""
    g = torch.Generator(device=dev).manual_seed(seed)
    re = torch.randn(batch, 512, tm, 2, device=dev, generator=g)
    im = torch.randn(batch, 512, tm, 2, device=dev, generator=g)
    gain = torch.exp(torch.rand(batch, 512, 1, 1, device=dev, generator=g) * 3.0 - 2.0)
    mix = torch.log1p(torch.sqrt(re * re + im * im) * gain).contiguous()
    tc = torch.randint(0, 11, (batch, 1), device=dev, generator=g)
    return mix, tc


DUMP_BUDGET_BYTES = 48 << 20


def dump_outputs(out_dir, outputs):
    """outputs: {name: device tensor with the batch first}.  Writes each as out_dir/<name>.npy in float32: whole when all of them fit in
    DUMP_BUDGET_BYTES, else the same seeded sample of batch rows (sorted) of each.  Returns the batch rows written."""
    batch = next(iter(outputs.values())).shape[0]
    per_row = sum(t[0].numel() * 4 for t in outputs.values())
    rows = torch.arange(batch)
    if per_row * batch > DUMP_BUDGET_BYTES:
        k = max(1, DUMP_BUDGET_BYTES // per_row)
        rows = torch.from_numpy(np.sort(np.random.default_rng(0).choice(batch, size=k, replace=False)))
    os.makedirs(out_dir, exist_ok=True)
    for name, t in outputs.items():
        np.save(os.path.join(out_dir, name + ".npy"), t[rows.to(t.device)].float().cpu().numpy())
    return rows.tolist()


def cpu_baseline(sd, tm, seconds):
    """The oracle timed on this host's cores.  PyTorch-CPU convs at batch 8 do not scale to hundreds of threads
    (256 threads ran 40x slower than 32 on the first GPU box), so a short probe picks the fastest thread count
    among {8,16,32,64,all}; `cores` reports the count actually used."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import m2h_oracle as O
    from m2h import synthetic
    ncpu = os.cpu_count() or 1
    bs = 8
    mixed, tc = synthetic.make_passive_inputs(bs, tm, 5)
    mix, tct = torch.from_numpy(mixed), torch.from_numpy(tc)

    def once():
        t = time.perf_counter()
        with torch.no_grad():
            O.passive_pair(sd, mix, tct)
        return time.perf_counter() - t

    best_t, best_n = None, None
    for n in sorted(set(min(c, ncpu) for c in (8, 16, 32, 64, ncpu))):
        torch.set_num_threads(n)
        once()  # warm-up (allocator, oneDNN primitive cache)
        t = min(once(), once())
        if best_t is None or t < best_t:
            best_t, best_n = t, n
        if t > 4 * best_t:
            break  # oversubscribed: larger counts only get worse
    torch.set_num_threads(best_n)
    _CPU_THREADS[0] = best_n
    t0 = time.perf_counter()
    n = 0
    while True:
        once()
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= 400:
            break
    return {"value": round(bs * n / el, 2), "unit": "spectrograms/s", "cores": best_n, "kind": "port",
            "sample": "%d batches of %d 512x%d spectrograms through oracle.passive_pair (PyTorch-CPU fp32, %d of %d host threads), %.1f s"
                      % (n, bs, tm, best_n, ncpu, el)}


_CPU_THREADS = [None]   # thread count the U-Net probe of cpu_baseline() picked on this host; the other CPU legs re-use it


def _cpu_threads():
    n = _CPU_THREADS[0]
    if n is None:
        n = min(32, os.cpu_count() or 1)
    torch.set_num_threads(n)
    return n


def ddppo_cpu_baseline(far_target, seconds):
    """The reference-CPU figure of the DD-PPO leg, timed in this run on this host: the oracle's restatement of the reference's
    training loop (oracle/m2h_oracle_trainer.py: collect_rollout_step = ppo_trainer.py:253-478, update_pol / update_sep =
    ppo.py:82-246; pinned to the reference's own PPOTrainer.train run by tests/golden/trainer_*.npz) over ONE sampled unit of
    each phase -- 20 rollout steps at 14 envs, one update_pol (4 epochs over the 280 stored samples), one update_sep EPOCH over
    a full 120-step buffer (1 680 samples) -- scaled by the schedule's counts per cycle (6 rollouts, 6 update_pol, 24 update_sep
    epochs): env-steps/s = 1 680 / (6 t_rollout + 6 t_update_pol + 24 t_sep_epoch).  The env is the host-side replay env
    (table lookups: zero-cost dynamics, like the GPU leg's).  What the reference's fps line (ppo_trainer.py:999-1001) would
    print for this schedule on these cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import m2h_oracle as O
    import m2h_oracle_trainer as OT
    from m2h import synthetic
    from m2h.envs.replay_env import ReplayHostVecEnv
    from m2h.rl.ppo.ppo_trainer import far_target_config, near_target_config
    ns = far_target_config() if far_target else near_target_config()
    cfg = dict(vars(ns))
    threads = _cpu_threads()
    N, T, C = cfg["NUM_PROCESSES"], cfg["num_steps"], cfg["num_updates_per_cycle"]
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in synthetic.make_state_dict(synthetic.policy_shapes(), 1).items()}
    for k in sd:
        if k.startswith(OT.POL_PREFIXES + OT.MEM_PREFIXES):
            sd[k].requires_grad_(True)
    opt_pol = torch.optim.Adam(OT._trainable(sd, OT.POL_PREFIXES), lr=cfg["lr_pol"], eps=cfg["eps"])
    opt_sep = torch.optim.Adam(OT._trainable(sd, OT.MEM_PREFIXES), lr=cfg["lr_sep"], eps=cfg["eps"])
    env = ReplayHostVecEnv(N, seed=cfg["SEED"], episode_len=cfg["MAX_EPISODE_STEPS"], pool=16, env_rewards=far_target)
    rk = OT.Rank(env, cfg)
    torch.manual_seed(0)
    OT.collect_rollout_step(sd, cfg, rk)          # the rollout's first step warms up (oneDNN primitive caches): not timed
    t0 = time.perf_counter()
    n_roll = 0
    for _ in range(T - 1):
        OT.collect_rollout_step(sd, cfg, rk)
        n_roll += 1
        if time.perf_counter() - t0 > seconds and n_roll >= 5:
            break                                    # slow host: fewer steps, same per-step figure
    t_step = (time.perf_counter() - t0) / n_roll
    while rk.ro.step != 0:                           # (a short sample leaves the storage part-filled: finish the rollout untimed)
        OT.collect_rollout_step(sd, cfg, rk)
    t0 = time.perf_counter()
    with torch.no_grad():                            # _update_pol (ppo_trainer.py:480-520)
        ro = rk.ro
        last = {kk: v[-1] for kk, v in ro.observations.items()}
        feats, _, _ = O.policy_net(sd, last, ro.recurrent_hidden_states_pol[-1], ro.masks[-1], ro.pred_binSepMasks[-1], ro.pred_mono[-1],
                                   ro.prev_pred_monoFromMem[-1])
        ro.compute_returns(O.heads(sd, feats)[0], cfg["use_gae"], cfg["gamma"], cfg["tau"])
    OT.update_pol(sd, opt_pol, [rk], cfg, cfg["clip_param"], True)
    rk.ro.after_update()
    t_pol = time.perf_counter() - t0
    # the separator storage holds T of its C*T steps after one rollout: tile them over the whole buffer (timing only)
    rs = rk.rs
    for name in ("prev_pred_monoFromMem", "masks"):
        buf = getattr(rs, name)
        for c in range(1, C):
            buf[c * T + 1:(c + 1) * T + 1].copy_(buf[1:T + 1])
    for buf in rs.observations.values():
        for c in range(1, C):
            buf[c * T + 1:(c + 1) * T + 1].copy_(buf[1:T + 1])
    one_epoch = dict(cfg, ppo_epoch=1)
    t0 = time.perf_counter()
    OT.update_sep(sd, opt_sep, [rk], one_epoch)
    t_sep = time.perf_counter() - t0
    cycle = C * T * t_step + C * t_pol + C * cfg["ppo_epoch"] * t_sep
    return {"value": round(C * T * N / cycle, 2), "unit": "env-steps/s", "cores": threads, "kind": "port",
            "s_per_cycle": round(cycle, 2), "rollout_step_s": round(t_step, 4), "update_pol_s": round(t_pol, 3), "update_sep_epoch_s": round(t_sep, 3),
            "sample": "oracle/m2h_oracle_trainer.py (PyTorch-CPU fp32 restatement of the reference's PPOTrainer loop, %d of %d host threads): "
                      "%d rollout steps at %d envs, one update_pol (%d epochs x %d samples), one update_sep epoch (%d samples), "
                      "scaled to the schedule's %d / %d / %d per cycle; %.1f s of CPU work"
                      % (threads, os.cpu_count() or 1, n_roll, N, cfg["ppo_epoch"], T * N, C * T * N, C * T, C, C * cfg["ppo_epoch"],
                         n_roll * t_step + t_pol + t_sep)}


def passive_train_cpu_baseline(tm, seconds, batch=8):
    """The oracle's passive training step (oracle.passive_train_step = passive_trainer.py:218-286 incl. D11: train-mode BatchNorm,
    both L1 losses, backward, Adam) at BASELINE config 1's batch of 8 on this host's cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import m2h_oracle as O
    from m2h import synthetic
    threads = _cpu_threads()
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in synthetic.make_state_dict(synthetic.passive_shapes(), 1).items()}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
    buffers = {k: v for k, v in sd.items() if "running_" in k}
    mixed, tc = synthetic.make_passive_inputs(batch, tm, 5)
    gen = torch.Generator().manual_seed(7)
    b = {"mixed_bin_audio_mag": torch.from_numpy(mixed), "target_class": torch.from_numpy(tc),
         "gt_bin_mag": torch.rand(batch, 512, tm, 2, generator=gen) * 2, "gt_mono_mag": torch.rand(batch, 512, tm, 1, generator=gen) * 2}
    _b, _m, opt = O.passive_train_step(params, buffers, b)   # warm-up
    t0 = time.perf_counter()
    n = 0
    while True:
        _b, _m, opt = O.passive_train_step(params, buffers, b, opt_state=opt)
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= 100:
            break
    return {"value": round(batch * n / el, 2), "unit": "spectrograms/s", "cores": threads, "kind": "port",
            "sample": "%d training steps of batch %d (512x%d) through oracle.passive_train_step (PyTorch-CPU fp32, %d of %d host threads), %.1f s"
                      % (n, batch, tm, threads, os.cpu_count() or 1, el)}


def ddppo_phase_rooflines(phase_ms, phase_launches, env_steps_per_cycle, sep_bf16x3, pol_bf16x3):
    """One roofline object per phase of the cycle, each against what bounds THAT phase, from this run's HIP events and launch counts only.
    rollout    : T x N env-steps of one frozen U-Net pair + AcousticMem + policy forward at 14 rows: nothing matrix-bound; the floor is
                 (kernel launches x 2 us, the price of a dependent kernel boundary, MI355X_MICROARCH.md) + (the step's weight set, 157.2 MB
                 of fp32 -- 33.47 M separator + 5.83 M policy parameters -- streamed once per step at the 6.3 TB/s a copy achieves);
    update_pol : ppo_epoch x (forward + backward ~ 3 x forward) of the policy over the 280 stored samples, fp32 (or bf16x3) MFMA;
    update_sep : ppo_epoch x AcousticMem forward + backward over the 1 680 stored samples (separator outputs cached), bf16x3 (or fp32)."""
    out = {}
    steps = env_steps_per_cycle
    if "rollout" in phase_ms:
        n = phase_launches.get("rollout")
        stream_ms = steps / 14.0 * 157.2e6 / 6.3e12 * 1e3           # one weight pass per rollout step (14 envs per step)
        floor = (n * 2e-3 if n else 0.0) + stream_ms
        out["rollout"] = {"bound": "kernel boundaries + weight stream", "ms_per_cycle": round(phase_ms["rollout"], 3), "m2h_kernel_launches_per_cycle": n,
                          "weight_stream_ms": round(stream_ms, 3), "launch_floor_ms": round(n * 2e-3, 3) if n else None,
                          "floor_ms": round(floor, 3), "frac": round(floor / phase_ms["rollout"], 4),
                          "achieved_weight_GBps": round(steps / 14.0 * 157.2e6 / (phase_ms["rollout"] * 1e-3) / 1e9, 1), "peak_GBps": 6300.0}
    if "update_pol" in phase_ms:
        gf = 6 * 4 * 3 * 0.0545 * 280
        peak = PEAK_BF16X3_TFLOPS if pol_bf16x3 else PEAK_F32_MFMA_TFLOPS
        ach = gf / phase_ms["update_pol"]
        out["update_pol"] = {"bound": "mfma", "ms_per_cycle": round(phase_ms["update_pol"], 3), "m2h_kernel_launches_per_cycle": phase_launches.get("update_pol"),
                             "gflop_per_cycle": round(gf, 1), "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                             "note": "24 epochs of ~170 launches over 280 rows: launch- and latency-bound far below the matrix peak (DESIGN 3.2c)"}
    if "update_sep" in phase_ms:
        gf = 24 * 3 * 0.0283 * steps
        peak = PEAK_BF16X3_TFLOPS if sep_bf16x3 else PEAK_F32_MFMA_TFLOPS
        ach = gf / phase_ms["update_sep"]
        out["update_sep"] = {"bound": "mfma", "ms_per_cycle": round(phase_ms["update_sep"], 3), "m2h_kernel_launches_per_cycle": phase_launches.get("update_sep"),
                             "gflop_per_cycle": round(gf, 1), "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4)}
    return out


def update_sep_kernel_rooflines(dev, samples, bf16x3):
    """Each of the conv / loss launches of one update_sep epoch (four in bf16x3 arithmetic, five in fp32) (AcousticMem forward + loss + backward over the stored samples,
    ppo.py:179-246; m2h/rl/models/memory_nets.py) launched alone on tensors of the epoch's shapes, HIP events around 5 launches in THIS run,
    bounded by what binds it: algorithmic bytes / time against the 6.3 TB/s a copy achieves, and algorithmic FLOP / time against the
    arithmetic's matrix ceiling (2500 / 3 TFLOP/s in bf16x3, 157.3 in fp32).  The phase's single MFMA fraction said nothing actionable:
    these kernels read and write 330-770 MB each for 14-32 GFLOP."""
    from m2h import functional as MF
    from m2h import ops
    g = torch.Generator(device=dev).manual_seed(3)
    B = int(samples)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x, h1, dh = r(B, 32, 32, 32), r(B, 32, 32, 32).relu_(), r(B, 32, 32, 32)
    dy = r(B, 32, 32, 16)
    gt_plane = r(B, 512, 32, 1)
    w0, w1 = r(32, 32, 3, 3) * 0.05, r(16, 32, 3, 3) * 0.05
    wp0, wp1 = ops.pack_conv_weight_ex(w0, 32, 32), ops.pack_conv_weight_ex(w1, 32, 32)
    wpd1 = MF.pack_dgrad_weight(w1, 1, 1)
    px = B * 32 * 32
    MB = 1e6
    cases = [
        ("forward conv 32->32 + ReLU", lambda: ops.conv2d_nhwc(x, wp0, 32, 3, 3, stride=1, pad=1, slope=0.0), 4.0 * px * (32 + 32), 2.0 * px * 32 * 288),
        ("forward conv 32->16 + L1 loss + its gradient (one launch: the conv's output is never stored)", lambda: ops.conv3x3_l1_nhwc16(h1, wp1, gt_plane),
         4.0 * px * (32 + 16 + 16), 2.0 * px * 16 * 288),
        ("weight gradient of conv 32->16", lambda: MF.conv_wgrad(h1, None, dy, 16, 3, 3, 1, 1, torch_ci=32), 4.0 * px * (32 + 16), 2.0 * px * 16 * 288),
    ]
    if bf16x3:   # conv0's weight gradient makes conv1's input gradient and the ReLU gate itself (m2h_conv_wgrad_dgrad_fused_f32): x + h (gate) + d loss / d y
        cases.append(("weight gradient of conv 32->32 with conv 32->16's input gradient + ReLU gate fused (the 32-channel gradient is never stored)",
                      lambda: MF.conv_wgrad_dgrad_fused(x, dy, wp1, h1, 0.0, 32), 4.0 * px * (32 + 32 + 16), 2.0 * px * 32 * 288 + 2.0 * px * 32 * 144))
    else:
        cases += [("input gradient of conv 32->16", lambda: MF.conv_dgrad(dy, w1, (32, 32), 1, 1, wp=wpd1), 4.0 * px * (16 + 32), 2.0 * px * 32 * 144),
                  ("weight gradient of conv 32->32 (ReLU gate fused)", lambda: MF.conv_wgrad(x, None, dh, 32, 3, 3, 1, 1, gate=h1, gate_slope=0.0, torch_ci=32),
                   4.0 * px * (32 + 32 + 32), 2.0 * px * 32 * 288)]
    peak_tf = PEAK_BF16X3_TFLOPS if bf16x3 else PEAK_F32_MFMA_TFLOPS
    out = {}
    with ops.math_scope(ops.MATH_BF16X3 if bf16x3 else ops.MATH_FP32), torch.no_grad():
        for name, fn, nbytes, flops in cases:
            fn()
            label = ops.last_kernel()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 5
            gbps, tf = nbytes / us / 1e3, flops / us / 1e6
            f_hbm, f_mfma = gbps / 6300.0, tf / peak_tf
            out[name] = {"kernel": label, "us": round(us, 1), "algorithmic_MB": round(nbytes / MB, 1), "achieved_GBps": round(gbps, 1), "frac_of_6300_GBps": round(f_hbm, 3),
                         "gflop": round(flops / 1e9, 2), "achieved_TFLOPs": round(tf, 1), "frac_of_matrix_ceiling": round(f_mfma, 3),
                         "bound": "hbm" if f_hbm >= f_mfma else "mfma"}
    out["what"] = ("one call each (the weight gradients: kernel + their split reduce) on tensors of the epoch's shapes (%d stored samples x 32 x 32 pixels), mean of 5 launches between two HIP events in this run; "
                   "the gate-fused weight gradient also reads the forward activation (three streams)") % B
    return out


def ddppo_roofline(env_steps_per_s_per_job, s_per_cycle, far_target, phase_ms_per_cycle=None):
    """Achieved-fraction object of the DD-PPO leg (BASELINE config 3 / 5).  FLOP figures per env-step: algorithmic = SURVEY 8d's
    reference schedule (13.8 GFLOP: 24 + 2 U-Net pair passes per env-step dominate); executed = what this build runs after the two
    result-preserving re-uses of DESIGN section 5 (separator outputs cached per stored observation: one pair pass per env-step in the
    rollout + one per stored sample per update_sep cycle, AcousticMem fwd+bwd x 24, policy fwd + 4 x fwd/bwd)."""
    algorithmic = 13.8
    # rollout: ONE pair pass + one memory pass per env-step (the next observation's outputs serve the following step) + policy forward;
    # update_pol: 4 epochs x (forward + backward ~ 3x forward); update_sep: one pair pass per stored sample per cycle (cached) +
    # 24 x AcousticMem forward + backward
    executed = (0.4226 + 0.0283 + 0.0545) + 4 * 3 * 0.0545 + (0.4226 + 24 * 3 * 0.0283)
    out = {"bound": "launch latency (kernels of 5-20 us at 14 rows; see DESIGN 3.2c)", "unit": "TFLOP/s",
           "algorithmic_gflop_per_env_step": algorithmic, "executed_gflop_per_env_step": round(executed, 3),
           "achieved_algorithmic": round(algorithmic * env_steps_per_s_per_job / 1e3, 2),
           "achieved": round(executed * env_steps_per_s_per_job / 1e3, 2), "peak": PEAK_F32_MFMA_TFLOPS,
           "frac": round(executed * env_steps_per_s_per_job / 1e3 / PEAK_F32_MFMA_TFLOPS, 4),
           "note": "per job (all ranks); peak = one GPU's fp32 MFMA peak x n_gpus is the fair ceiling at N > 1"}
    # phase_time_share: the three phases' HIP-event time on the compute stream over this run's own wall time per cycle (both measured
    # here; what is missing from 1 is host time with an idle device).  The per-phase objects (`phases`, ddppo_phase_rooflines) carry
    # this run's own launch counts and bound every phase by what bounds it; nothing here is read from a committed profile.
    if phase_ms_per_cycle is not None:
        out["phase_ms_per_cycle"] = round(phase_ms_per_cycle, 3)
        out["phase_time_share"] = round(min(1.0, phase_ms_per_cycle / (1e3 * s_per_cycle)), 3)
    return out


def run_ddppo(args, dev, rank, world, dist, far_target=False, with_cpu=False):
    """Second figure of BASELINE.json's metric: DD-PPO env-steps/s on the reference schedule (nearTarget.yaml: 14 envs/rank,
    T=20, 6 policy updates + 6 separator updates per cycle, 4 epochs, 1 minibatch) with the synthetic on-device env.
    Whole-job rate = all ranks' env steps / max-over-ranks time; gradients are all-reduced over RCCL when world > 1.
    far_target: BASELINE config 5 -- farTarget.yaml (episodes of 80 steps, the environment's navigation reward, no reward
    override) with the forward / input-gradient GEMMs in bf16x3 math (the build-side mixed-precision mode); the
    distance of that arithmetic from the fp32 one is measured on one evaluate_actions batch and reported beside the rate."""
    from m2h import ops
    from m2h.rl.ppo.ppo_trainer import PPOTrainer, far_target_config, near_target_config
    syn = __import__("m2h.synthetic", fromlist=["x"])
    tail = bool(args.tail_overlap)
    force = dict(bucketed_grad_reduce=True, overlap_grad_reduce=True) if args.force_buckets else {}
    if args.force_schedule:
        force = dict(overlap_grad_reduce=True) if args.force_schedule == "overlap" else dict(bucketed_grad_reduce=True)
    cfg = (far_target_config(rollout_math="fp32", overlap_update_tail=tail, **force) if far_target
           else near_target_config(sep_update_math=args.sep_update_math, overlap_update_tail=tail, **force))
    ops.set_math_mode(ops.MATH_BF16X3 if far_target else ops.MATH_FP32)
    try:
        tr = PPOTrainer(cfg, dev, world_rank=rank, world_size=world)
        tr.setup()
        tr.actor_critic.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_state_dict(syn.policy_shapes(), 1).items()})
        from m2h.rl.ppo import ddppo_utils
        tr.train_cycle()  # warm-up (allocator, pack caches, lazy optimizer buffers, graph capture)
        tr.train_cycle()  # ... and a second one: the leg starts after ~15 s of host-only work (the CPU baseline) with the device idle
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        phase_events = []
        coll = ddppo_utils.collective_log(True)
        t0 = time.perf_counter()
        steps = 0
        last = None
        for _ in range(args.ddppo_cycles):
            last = tr.train_cycle(phase_events=phase_events)
            steps += last["env_steps"]
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        ddppo_utils.collective_log(False)
        if dist is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        # per-cycle phase times on the compute stream and the gradient all-reduces wherever they ran (compute or side stream)
        phases, launches = {}, {}
        for name, e0, e1 in phase_events:
            phases[name] = phases.get(name, 0.0) + e0.elapsed_time(e1)
            launches[name] = launches.get(name, 0) + (e1.m2h_kernels - e0.m2h_kernels)
        launches = {k: int(round(v / args.ddppo_cycles)) for k, v in launches.items()}
        if tail and "update_pol" in launches and "update_sep" in launches:
            launches["update_pol"] -= launches["update_sep"]   # (the tail's separator updates are enqueued inside the last update_pol's bracket)
        breakdown = {k + "_ms": round(v / args.ddppo_cycles, 3) for k, v in phases.items()}
        breakdown["grad_allreduce_ms"] = round(sum(e0.elapsed_time(e1) for e0, e1, _b, _x in coll) / args.ddppo_cycles, 3)
        # exposed: the all-reduces enqueued on the compute stream (it waits for them before clip + Adam); the others run on the side stream
        # under the encoders' backward (first bucket of every policy epoch) or under the next phase (the last step of every update)
        breakdown["grad_allreduce_exposed_ms"] = round(sum(e0.elapsed_time(e1) for e0, e1, _b, x in coll if x) / args.ddppo_cycles, 3)
        breakdown["grad_allreduce_exposed_count"] = sum(1 for _e0, _e1, _b, x in coll if x) // max(1, args.ddppo_cycles)
        breakdown["grad_allreduce_count"] = len(coll) // max(1, args.ddppo_cycles)
        breakdown["grad_allreduce_payload_bytes"] = sorted({b for _e0, _e1, b, _x in coll}, reverse=True)
        pol_bytes = tr.agent.optimizer_pol.flat_g.numel() * 4
        breakdown["policy_grad_bytes"] = pol_bytes
        # one stand-alone all-reduce of the policy's flat gradient size, timed alone (RCCL over xGMI when world > 1)
        standalone_us = 0.0
        if dist is not None:
            buf = torch.zeros(pol_bytes // 4, device=dev)
            for _ in range(2):
                dist.all_reduce(buf)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                dist.all_reduce(buf)
            e1.record()
            torch.cuda.synchronize()
            standalone_us = 1e3 * e0.elapsed_time(e1) / 5
            del buf
        breakdown["allreduce_23MB_us"] = round(standalone_us, 1)
        if tail:
            breakdown["overlap"] = ("the cycle's six update_sep run on a second HIP stream beside the sixth update_pol (same results, tests/test_gpu_round4.py): "
                                    "update_sep_ms is measured on that stream and overlaps the last sixth of update_pol_ms, so the three phases sum to more than the cycle")
        breakdown["what"] = ("HIP-event time per cycle of the three phases on the compute stream (6 x rollout of 20 steps, 6 x update_pol, 6 x update_sep) and of the "
                             "flat-gradient all-reduces on the stream each ran on (the last one of every update on the side stream, under the next phase); "
                             "allreduce_23MB_us = a stand-alone all-reduce of the policy gradient's size; all zero-collective at one rank")
        props = torch.cuda.get_device_properties(dev)
        ident = {"rank": rank, "device_index": dev.index, "name": props.name, "uuid": str(getattr(props, "uuid", "")),
                 "pci_bus_id": "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0), getattr(props, "pci_device_id", 0))}
        if dist is not None:
            idents = [None] * world
            dist.all_gather_object(idents, ident)
        else:
            idents = [ident]
        # the same cycles once more with action_sampling="cpu_generator" -- the mode every reference-pinned trainer test samples in (noise from
        # the CPU default generator at the reference's stream position: the reference PyTorch-CPU run's actions from the seed alone); the
        # default "fused" mode is pinned end to end by the recorded-noise test of tests/test_gpu_trainer_golden.py.  Same kernels but the
        # draw's noise source: one pinned host->device copy per step instead of the in-kernel Philox draw.
        default_sampling = tr.actor_critic._sampling_mode
        tr.actor_critic.set_action_sampling("cpu_generator")
        tr.train_cycle()   # (the rollout graphs are captured anew: another draw)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        steps_cg = sum(tr.train_cycle()["env_steps"] for _ in range(args.ddppo_cycles))
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el_cg = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el_cg], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el_cg = float(t.item())
        sampling_modes = {"default": default_sampling,
                          default_sampling: {"value": round(world * steps / el, 1), "s_per_cycle": round(el / args.ddppo_cycles, 4)},
                          "cpu_generator": {"value": round(world * steps_cg / el_cg, 1), "s_per_cycle": round(el_cg / args.ddppo_cycles, 4)},
                          "unit": "env-steps/s",
                          "what": ("the headline value of this leg is the default mode's; cpu_generator = the bit-exact-from-the-seed mode of the "
                                   "reference-pinned tests, same cycles in this same run")}
        mixed = None
        if far_target:
            # the same evaluate_actions batch (the policy storage as it stands) in both arithmetic modes
            ro, ac = tr.rollouts_pol, tr.actor_critic
            flat = lambda x: x.reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:]))  # noqa: E731
            obs = {k: flat(v[:-1]) for k, v in ro.observations.items()}
            outs = []
            for mode in (ops.MATH_FP32, ops.MATH_BF16X3):
                ops.set_math_mode(mode)
                with torch.no_grad():
                    v, lp, _ent, _h = ac.evaluate_actions(obs, ro.recurrent_hidden_states_pol[0], flat(ro.masks[:-1]), flat(ro.actions),
                                                          pred_binSepMasks=flat(ro.pred_binSepMasks), pred_mono=flat(ro.pred_mono),
                                                          pred_monoFromMem=flat(ro.prev_pred_monoFromMem[1:]))
                outs.append((v.clone(), lp.clone()))
            rel = lambda a, b: float(((a - b).abs().sum() / b.abs().sum()).item())  # noqa: E731
            mixed = {"what": "rel-L1 of evaluate_actions (280 stored samples) in bf16x3 math against fp32 math, same weights and inputs",
                     "value": rel(outs[1][0], outs[0][0]), "action_log_probs": rel(outs[1][1], outs[0][1])}
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    out = {"metric": "ddppo_env_steps_per_sec", "value": round(world * steps / el, 1), "unit": "env-steps/s", "n_gpus": world,
           "cycles": args.ddppo_cycles, "s_per_cycle": round(el / args.ddppo_cycles, 4), "envs_per_rank": cfg.NUM_PROCESSES,
           "schedule": ("farTarget.yaml: episodes of 80 steps, navigation reward (no override), " if far_target else "nearTarget.yaml: ") +
                       "T=20, 6x(rollout+update_pol) + 6x update_sep per cycle, ppo_epoch 4, 1 minibatch, hidden 512",
           "env": "synthetic on-device env (cached 128x128 RGB-D frames + spectrogram pool), zero-cost dynamics",
           "action_sampling": default_sampling, "action_sampling_modes": sampling_modes,
           "launch": ("HIP graphs: the rollout step (one graph per (extra-reward, episode-end) flag pair, one chain) and the update_pol epoch "
                      "(forward + losses + backward; the three encoders as parallel branches, launched onto a drained stream: DESIGN 3.2h) are "
                      "captured once and replayed, and so is the update_sep epoch (one chain); optimizer steps and collectives are enqueued kernel by kernel" if cfg.use_hip_graphs else "kernel by kernel"),
           "grad_reduce": ("sum all-reduce (RCCL) of the policy's flat gradient in two buckets per backward: recurrent encoder + heads on a side stream "
                           "under the encoders' backward, then the encoders' bucket; one flat all-reduce for the acoustic memory; the last all-reduce + "
                           "clip + Adam of every update runs on the side stream, fenced at the next reader of those parameters" if world > 1 else "single rank: no collective"),
           "separator_output_reuse": "frozen eval-mode U-Net outputs computed once per stored observation and re-used by the 24 "
                                     "update_sep passes and by the next rollout step (result-preserving; SURVEY D13)",
           "last_pol_losses": [round(x, 5) for x in last["pol_losses"]], "last_sep_losses": [round(x, 5) for x in last["sep_losses"]],
           "phases": breakdown, "devices": idents, "distinct_devices": len({(d["uuid"], d["pci_bus_id"]) for d in idents}),
           "roofline": ddppo_roofline(world * steps / el, el / args.ddppo_cycles, far_target,
                                      sum(phases.values()) / args.ddppo_cycles if phases else None)}
    out["roofline"]["m2h_kernel_launches_per_cycle"] = sum(launches.values()) if launches else None
    out["roofline"]["phases"] = ddppo_phase_rooflines({k: v / args.ddppo_cycles for k, v in phases.items()}, launches, steps / args.ddppo_cycles,
                                                      sep_bf16x3=far_target or args.sep_update_math == "bf16x3", pol_bf16x3=far_target)
    if rank == 0 and world == 1 and "update_sep" in out["roofline"]["phases"]:
        # per kernel, each against what binds it (the phase's own fraction stays beside them for continuity with earlier rounds)
        out["roofline"]["phases"]["update_sep"]["kernels"] = update_sep_kernel_rooflines(
            dev, steps / args.ddppo_cycles, far_target or args.sep_update_math == "bf16x3")
    del tr
    if with_cpu:   # rank 0 at N = 1 only: the oracle's loop on this host's cores, in this same run (bounded sample)
        out["cpu_baseline"] = ddppo_cpu_baseline(far_target, args.cpu_seconds)
        out["speedup_vs_cpu_baseline"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
    if far_target:
        out["math"] = ("mixed: bf16x3 products (fp32 tensors and accumulation) in the forward / input-gradient GEMMs of update_pol and update_sep; fp32 in the "
                       "14-env rollout steps (launch- and latency-bound: nothing matrix-bound to save there, and that batch's one-launch kernels are fp32), "
                       "weight gradients, reductions, Adam")
        out["mixed_precision_parity"] = mixed
    else:
        out["math"] = ("fp32 MFMA / fp32 everywhere" if args.sep_update_math == "fp32" else
                       "fp32 (MFMA and vector) in the rollout steps and update_pol; update_sep's AcousticMem convolutions, input gradient and weight gradients "
                       "over the 1680 stored samples in bf16x3 (split bf16 products, fp32 tensors and accumulation: ~6e-6 rel-L1 from the fp32 kernels, "
                       "tests/test_gpu_round4.py); --sep-update-math fp32 runs them on the fp32 matrix pipe")
    return out


def run_feeder(args, dev, rank, with_cpu):
    """Row N1 of SURVEY 8f: the waveform -> spectrogram feeder (RIR convolution, int16 round trip, mixing, three STFTs, RMS
    normalisation; pretrain/datasets/dataset.py:162-228) on the GPU, batch = pretrain_passive.yaml's 64 clips of 1 s with two
    sources each, synthetic audio of SURVEY 8d; beside it the numpy / scipy restatement of the same function on one host core
    (the reference runs it on 60 loader workers)."""
    from m2h.audio.feeder import BinauralFeeder
    B, S, L, Lr = args.feeder_batch, 2, 16000, 16000
    g = torch.Generator(device=dev).manual_seed(11 + rank)
    mono = torch.clamp(torch.round(3000 * torch.randn(B, S, L, device=dev, generator=g)), -32768, 32767)
    t = torch.arange(Lr, device=dev) / 16000.0
    rir = torch.randn(B, S, Lr, 2, device=dev, generator=g) * torch.exp(-t / 0.05)[None, None, :, None]
    rir = rir / rir.abs().amax(dim=(2, 3), keepdim=True) * 0.05
    fd = BinauralFeeder(dev, gt_mono_mag_norm=1.2)
    for _ in range(2):
        fd.compute_audiospects(mono, rir)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.feeder_steps):
        out = fd.compute_audiospects(mono, rir)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res = {"metric": "feeder_clips_per_sec", "value": round(B * args.feeder_steps / el, 1), "unit": "1-s binaural clips/s", "batch": B,
           "ms_per_batch": round(1e3 * el / args.feeder_steps, 3), "sources_per_clip": S, "out": [list(o.shape) for o in out],
           "what": "BinauralFeeder.compute_audiospects: fftconvolve-same (hand-written in-LDS FFTs, m2h_fftconv_full) of 2 sources x 2 ears, round -> int16 -> /32768, source mean, "
                   "STFT(1023, 512) x 3 with |.|, log1p on the mixture, RMS-normalised GT mono magnitude"}
    if with_cpu:   # (the oracle is imported by this cpu_baseline leg only)
        if os.path.join(ROOT, "oracle") not in sys.path:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import m2h_oracle as O
        mono_h, rir_h = mono[:4].cpu().numpy(), rir[:4].cpu().numpy()
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 3.0:
            O.np_compute_audiospects(mono_h[n % 4], rir_h[n % 4], 1.2)
            n += 1
        res["cpu_baseline"] = {"value": round(n / (time.perf_counter() - t0), 1), "unit": "1-s binaural clips/s", "cores": 1, "kind": "port",
                               "sample": "%d clips through oracle.np_compute_audiospects (numpy / scipy restatement), one thread" % n}
    return res


def run_passive_train(args, dev, rank, with_cpu=False):
    """Secondary figure of SURVEY 8d config 2: the passive pre-training step (train-mode BN forward, U-Net backward, Adam) on
    the reference's batch (pretrain_passive.yaml: 64 clips of 512x32) with the synthetic feeder; replicas only across GPUs
    (train-mode BN), so every rank runs the same-size job and the rate is per replica."""
    from m2h import ops
    from m2h.pretrain.passive.passive_trainer import PassiveTrainer, passive_config
    cfg = passive_config(BATCH_SIZE=args.train_batch, TM=args.train_tm, SEED=3 + rank)
    ops.set_math_mode(ops.MATH_BF16X3 if args.train_math == "bf16x3" else ops.MATH_FP32)
    try:
        tr = PassiveTrainer(cfg, dev)
        tr.setup()
        batch = tr.feeders["train"].batch()
        for _ in range(2):
            tr.train_batch(*batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.train_steps):
            losses = tr.train_batch(*batch)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    finally:
        ops.set_math_mode(ops.MATH_FP32)
    gf = (0.4226 if args.train_tm == 32 else 0.4226 * args.train_tm / 32) * 3.0   # training step ~ 3x the forward
    ach = gf * args.train_batch * args.train_steps / el / 1e3
    peak = PEAK_F32_MFMA_TFLOPS if args.train_math == "fp32" else 2500.0 / 3.0
    out = {"metric": "passive_train_spectrograms_per_sec", "value": round(args.train_batch * args.train_steps / el, 1),
           "unit": "spectrograms/s", "ms_per_step": round(1e3 * el / args.train_steps, 3), "batch": args.train_batch,
           "time_frames": args.train_tm, "steps": args.train_steps, "math": args.train_math,
           "algorithmic_tflops": round(ach, 2),
           "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                        "algorithmic_gflop_per_step": round(gf * args.train_batch, 2),
                        "what": "algorithmic FLOP of the step (SURVEY 8d: 3 x the pair forward, 1.27 GFLOP per 512x32 clip) over the whole step's wall "
                                "time (forward, BatchNorm statistics, backward, Adam), against the dense MFMA peak of the step's GEMM arithmetic"},
           "last_losses": [round(float(x), 5) for x in losses],
           "what": "PassiveTrainer.train_batch: both U-Nets forward in train-mode BN, L1 losses, full backward, FlatAdam step",
           "launch": "one HIP graph per step: weight packs, forward, losses, backward and Adam of the two networks as two branches (the mono separator reads the "
                     "binaural masks detached), launched onto a drained stream (DESIGN 3.2h); M2H_PARALLEL_BRANCHES=0 = one chain"}
    del tr
    if with_cpu:
        out["cpu_baseline"] = passive_train_cpu_baseline(args.train_tm, min(args.cpu_seconds, 8.0))
        out["speedup_vs_cpu_baseline"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
    return out


def spawn_ranks(n):
    """``python bench.py --gpus N`` without a launcher: start N copies of this command, one rank per GPU, with the env-var rendezvous
    torch.distributed.run would provide (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT: what the reference's
    init_distrib_slurm reads, ddppo_utils.py:117-165).  Runs BEFORE anything in this process touches the GPU; this process only
    waits.  Rank 0 prints the one JSON line on the inherited stdout.  Returns the exit code (non-zero if any rank failed)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    pending = list(procs)
    while pending:
        for p in list(pending):
            code = p.poll()
            if code is None:
                continue
            pending.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in pending:   # a failed rank leaves the others blocked in a collective: stop exactly the children started here
                    q.terminate()
        time.sleep(0.2)
    return rc


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X: the m2h ops have no CPU path")
    # rehearsal knobs (tests / one-GPU boxes only): M2H_BENCH_DEVICE pins every rank to one card, M2H_BENCH_BACKEND=gloo replaces
    # RCCL (two ranks cannot share a GPU under RCCL); the driver's runs use neither
    dev = torch.device("cuda", int(os.environ.get("M2H_BENCH_DEVICE", local_rank)))
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("M2H_BENCH_BACKEND", "nccl")
        dist.init_process_group(backend, rank=rank, world_size=world, **({"device_id": dev} if backend == "nccl" else {}))
    ranks_observed = dist.get_world_size() if dist is not None else 1
    if ranks_observed != args.gpus:
        raise RuntimeError("bench.py --gpus %d but the process group has %d rank(s) (WORLD_SIZE=%s)" % (args.gpus, ranks_observed, os.environ.get("WORLD_SIZE")))

    from m2h import ops
    for kv in filter(None, args.knobs.split(",")):
        ops.debug_set(int(kv.split("=")[0]), int(kv.split("=")[1]))
    if args.knobs:
        from m2h import functional as MF_
        MF_.carry_tuning(True)   # (backward passes run on autograd's thread: they take the knobs of the forward's thread along)
    pol, sd = make_policy(dev)
    mix, tc = make_inputs(dev, args.batch, args.tm, 1000 + rank)
    obs = {"mixed_bin_audio_mag": mix, "target_class": tc}

    from m2h.graphs import GraphedSeparatorPair
    graphed = None if args.no_graph else GraphedSeparatorPair(pol, obs)

    def step():
        """one pass of the pair over the resident batch; by default replayed from a HIP graph (the same kernels, captured
        once per arithmetic mode) -- --no-graph enqueues them through the two m2h_unet_fwd calls instead"""
        if graphed is not None:
            return graphed()
        with torch.no_grad():
            masks = pol.get_binSepMasks(obs)
            mono = pol.convert_bin2mono(masks, mixed_audio=mix)
        return masks, mono

    from m2h.rl.models.separator_cnn import unet_forward, UNET_KERNEL_NAMES

    def stage_labels(mode):
        """The kernel each of the 11 stages of both U-Nets really launches at this shape, asked of the library (m2h_unet_fwd_stage_kernel)."""
        ops.set_math_mode(ops.MATH_BF16X3 if mode == "bf16x3" else ops.MATH_FP32)
        out = {}
        with torch.no_grad():
            enc, dec = pol.binSep_enc.passive_sep_encoder, pol.binSep_dec.passive_sep_decoder
            masks = unet_forward(enc, dec, mix, None, tc)
            out["binSep"] = ops.unet_stage_kernels()
            enc, dec = pol.bin2mono_enc.passive_sep_encoder, pol.bin2mono_dec.passive_sep_decoder
            unet_forward(enc, dec, mix, masks)
            out["bin2mono"] = ops.unet_stage_kernels()
        return out

    def unet_kernel_meta(n_out, with_masks, with_class, labels):
        """(name, kernel label, M, N, K, algorithmic flops, algorithmic bytes) of the 11 stages of one U-Net at this batch."""
        B, T = args.batch, args.tm
        fused0 = labels[0].startswith("(no launch")           # the strip kernel takes the slice and the first stage together
        in_bytes = (2 if with_masks else 1) * B * 512 * T * 2 * 4.0
        metas = [("sep_slice_input", labels[0], None, None, None, 0.0, 0.0 if fused0 else in_bytes + B * 512 * T * 2 * 4.0)]
        enc = [32, 64, 128, 256, 512, 512]
        H, W = 32, T
        for i in range(5):
            M, N, K = B * (H // 2) * (W // 2), enc[i + 1], 16 * enc[i]
            fl = 2.0 * M * N * 16 * (enc[i] + (1 if (i == 0 and with_class) else 0))
            by = 4.0 * (B * H * W * enc[i] + M * N + N * K)
            if i == 0 and fused0:
                by = in_bytes + 4.0 * (M * N + N * K)
            metas.append(("unet_down_fwd", labels[1 + i], M, N, K, fl, by))
            H //= 2
            W //= 2
        c0, c1, co = [512, 512, 256, 128, 64], [0, 512, 256, 128, 64], [512, 256, 128, 64, n_out]
        for i in range(5):
            M, N, K = 4 * B * H * W, co[i], 4 * (c0[i] + c1[i])
            fl = 2.0 * M * N * (K + (N if i == 4 else 0))                    # last stage carries the 1x1 head
            outel = M * N if i < 4 else B * 512 * T * (n_out // 16)
            by = 4.0 * (B * H * W * (c0[i] + c1[i]) + outel + 4 * N * K)
            metas.append(("unet_up_fwd" if i < 4 else "unet_up_head_fwd", labels[6 + i], M, N, K, fl, by))
            H *= 2
            W *= 2
        return metas

    META = {}
    for m_ in (() if not args.full else (args.math,) if args.no_other_mode else ("bf16x3", "fp32")):
        lab = stage_labels(m_)
        META[m_] = {"binSep": unet_kernel_meta(32, False, True, lab["binSep"]), "bin2mono": unet_kernel_meta(16, True, False, lab["bin2mono"])}
    ops.set_math_mode(ops.MATH_FP32)
    current_mode = [args.math]

    def step_events(sink):
        """the same pair through the same one-call runner, which records an event around each of its 11 kernels"""
        evs = []
        with torch.no_grad():
            for which in ("binSep", "bin2mono"):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(12)]
                for e in ev:
                    e.record()
                evs.append(ev)
            enc, dec = pol.binSep_enc.passive_sep_encoder, pol.binSep_dec.passive_sep_decoder
            masks = unet_forward(enc, dec, mix, None, tc, events=evs[0])
            enc, dec = pol.bin2mono_enc.passive_sep_encoder, pol.bin2mono_dec.passive_sep_decoder
            mono = unet_forward(enc, dec, mix, masks, events=evs[1])
        for which, ev in zip(("binSep", "bin2mono"), evs):
            for i, (name, inst, M, N, K, fl, by) in enumerate(META[current_mode[0]][which]):
                sink.append((name, {"kernel": inst, "M": M, "N": N, "K": K, "flops": fl, "bytes": by}, ev[i], ev[i + 1]))
        return masks, mono

    PEAK_BF16 = 2500.0   # dense bf16 MFMA peak, TFLOP/s (MI355X_MICROARCH.md)

    def timed_run(mode, steps, warmup, with_events):
        """W untimed + K timed steps of the pair in the given math mode -> (elapsed s, HIP-event sink or None, last step's outputs)."""
        ops.set_math_mode({"bf16x3": ops.MATH_BF16X3, "bf16": ops.MATH_BF16}.get(mode, ops.MATH_FP32))
        current_mode[0] = mode if mode != "bf16" else "bf16x3"   # (the hi-halves-only mode runs the bf16x3 mode's engines)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        sink = [] if with_events else None
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = None
        for _ in range(steps):
            if with_events:
                out = step_events(sink)
            else:
                out = step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, sink, out

    def account(sink, steps, mode):
        """per-kernel accounting from the HIP events of a timed region -> (roofline dict, per-layer dict)"""
        fam, per_layer = {}, {}
        for name, meta, e0, e1 in sink:
            ms = e0.elapsed_time(e1)
            k = meta.get("kernel", name)
            f = fam.setdefault(k, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
            f["ms"] += ms
            f["flops"] += meta.get("flops", 0.0)
            f["bytes"] += meta.get("bytes", 0.0)
            f["launches"] += 1
            key = "%s M=%s N=%s K=%s" % (name, meta.get("M"), meta.get("N"), meta.get("K"))
            pl = per_layer.setdefault(key, {"ms": 0.0, "flops": 0.0, "n": 0})
            pl["ms"] += ms
            pl["flops"] += meta.get("flops", 0.0)
            pl["n"] += 1
        igemm = {k: v for k, v in fam.items() if v["flops"] > 0}   # every conv kernel (the implicit-GEMM engines and the strip walkers)
        tot_ms = sum(v["ms"] for v in igemm.values())
        tot_fl = sum(v["flops"] for v in igemm.values())
        dom = max(igemm.items(), key=lambda kv: kv[1]["ms"])
        ach = tot_fl / (tot_ms * 1e-3) / 1e12
        # HBM traffic of the dominant instantiation: PMC counters cannot be read from inside this process, so the per-launch
        # figure of the committed rocprofv3 --pmc passes over this same command is reported (null when the file is absent)
        traffic, traffic_src = None, None
        tpath = next((q for q in (os.path.join(ROOT, "profiles", "r%02d_pmc_hbm_traffic.json" % r) for r in (6, 5, 4, 3, 2, 1)) if os.path.exists(q)), None)
        if tpath is not None:
            with open(tpath) as f:
                tj = json.load(f).get(mode, {})
            traffic, traffic_src = tj.get("traffic_bytes_per_launch"), tj.get("source")
        if mode == "bf16x3":
            # every algorithmic product is three bf16 MFMA products: the ceiling of this formulation is a third of the bf16 peak
            peak = PEAK_BF16 / 3.0
            kern = ("the conv kernels of csrc/ in bf16x3 math on split32 operands (fp32 values as bf16 hi + lo pairs; "
                    "hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16, fp32 accumulate): m2h::igemm_patch_kernel "
                    "(shared-patch LDS-DMA engine, 256x128 and 512x64 tiles: the wide stages and the 64-wide transposed stage), "
                    "m2h::igemm_dma_kernel<256,128> (LDS-DMA engine, two K-halves: the fourth encoder stage), m2h::igemm_f32_kernel<..., SPLIT=2> "
                    "(register-staged engine: the deepest stages), m2h::conv1_strip_kernel / m2h::convT_last_strip_kernel (strip walkers: "
                    "slice + first stage, last stage + head); `achieved` is over all of them, `dominant_instantiation` the one with the largest "
                    "share of the step; labels come from the library (m2h_unet_fwd_stage_kernel)")
        else:
            peak = PEAK_F32_MFMA_TFLOPS
            kern = "m2h::igemm_f32_kernel (all instantiations; MFMA f32 32x32x2 / 16x16x4 implicit-GEMM conv)"
        roofline = {
            "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "traffic": traffic,
            "traffic_unit": "HBM bytes per launch of the dominant instantiation (2*FETCH_SIZE + WRITE_SIZE)", "traffic_source": traffic_src,
            "kernel": kern,
            "launches_per_step": sum(v["launches"] for v in igemm.values()) // steps,
            "kernel_ms_per_step": round(tot_ms / steps, 4),
            "algorithmic_gflop_per_step": round(tot_fl / steps / 1e9, 3),
            "dominant_instantiation": {
                "name": dom[0], "avg_launch_us": round(1e3 * dom[1]["ms"] / dom[1]["launches"], 2),
                "launches_per_step": dom[1]["launches"] // steps,
                "achieved_tflops": round(dom[1]["flops"] / (dom[1]["ms"] * 1e-3) / 1e12, 2)},
            "by_instantiation": {k: {"ms_per_step": round(v["ms"] / steps, 4), "launches_per_step": v["launches"] // steps,
                                     "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["flops"] else None,
                                     "algorithmic_GBps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)}
                                 for k, v in fam.items()},
        }
        if mode == "bf16x3":
            roofline["peak_note"] = "bf16 dense MFMA peak 2500 TFLOP/s / 3 MFMA products per algorithmic product"
            roofline["executed_bf16_mfma_tflops"] = round(3.0 * ach, 1)
            roofline["frac_of_fp32_mfma_peak"] = round(ach / PEAK_F32_MFMA_TFLOPS, 3)
        layers = {k: {"us": round(1e3 * v["ms"] / v["n"], 1), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["flops"] else None}
                  for k, v in per_layer.items()}
        return roofline, layers

    # the headline run, then the other arithmetic beside it (fewer steps), then the distance between the two results
    # Headline pass: W warm-up + K timed steps with each U-Net enqueued by ONE C call (m2h_unet_fwd: what every RL call site
    # runs).  Kernel durations for the roofline come from a second pass of the same K steps through the same runner with an
    # event recorded around each of its kernels (m2h_unet_fwd_events): identical kernels, ~24 extra event records per step.
    other = "fp32" if args.math == "bf16x3" else "bf16x3"
    elapsed, _, last_out = timed_run(args.math, args.steps, args.warmup, False)
    if args.dump_outputs and rank == 0:
        # (before any other pass: the graph replays return their static output buffers)
        dump_outputs(args.dump_outputs, {"pred_binSepMasks": last_out[0], "pred_mono": last_out[1]})
    del last_out
    roofline, layers, evented_ms = None, None, None
    if args.full and not args.no_kernel_timing:
        # the per-kernel pass enqueues kernel by kernel with an event around each: when the host is slow (a busy box) the device idles between
        # the kernels, clocks down, and every duration reads high (seen: 8.4 ms per evented step, kernels +15 %).  Up to three passes; the one
        # whose wall time is closest to the graph replay's is kept, and the number of passes is reported.
        # The FIRST pass is the one reported unless it was host-bound (wall > 1.25 x the graph replay's): then the pass is repeated, up to three
        # in all, and the first that is not host-bound is taken (none: the fastest, flagged).  Every pass's wall time is in the line.
        passes = []
        for attempt in range(3):
            passes.append(timed_run(args.math, args.steps, 1, True)[:2])
            if passes[-1][0] <= 1.25 * elapsed:
                break
        host_bound = passes[-1][0] > 1.25 * elapsed
        pick = len(passes) - 1 if not host_bound else min(range(len(passes)), key=lambda i: passes[i][0])
        ev_elapsed, sink = passes[pick]
        roofline, layers = account(sink, args.steps, args.math)
        evented_ms = round(1e3 * ev_elapsed / args.steps, 3)
        roofline["evented_pass_ms_per_step"] = evented_ms
        roofline["evented_passes_run"] = len(passes)
        roofline["evented_passes_ms_per_step"] = [round(1e3 * e / args.steps, 3) for e, _s in passes]
        roofline["evented_pass_selected"] = pick
        roofline["evented_pass_host_bound"] = bool(host_bound)
        # `achieved` / `frac` are over the TIMED step (what the driver's clock sees: graph replay, launch gaps included); the evented pass's
        # kernel-time sum gives the per-kernel figures and is kept beside them
        roofline["achieved_kernel_sum"], roofline["frac_kernel_sum"] = roofline["achieved"], roofline["frac"]
        step_tflops = roofline["algorithmic_gflop_per_step"] / (1e3 * elapsed / args.steps)
        roofline["achieved"] = round(step_tflops, 2)
        roofline["frac"] = round(step_tflops / roofline["peak"], 4)
        roofline["achieved_what"] = ("algorithmic GFLOP of one step / ms_per_step of the timed region (HIP-graph replay); achieved_kernel_sum / frac_kernel_sum: "
                                     "the same GFLOP over the sum of the conv kernels' HIP-event durations in the evented pass")
    other_mode, parity, bf16_mode = None, None, None
    if args.full and not args.no_other_mode:
        o_steps = max(2, args.steps // 3)
        o_elapsed, _, _ = timed_run(other, o_steps, 1, False)
        o_roof = None
        if not args.no_kernel_timing:
            _e, o_sink, _ = timed_run(other, o_steps, 1, True)
            o_roof, _ = account(o_sink, o_steps, other)
        ops.set_math_mode(ops.MATH_FP32)
        m_a, mono_a = (t.clone() for t in step())  # (graph replays return their static output buffers)
        ops.set_math_mode(ops.MATH_BF16X3)
        m_b, mono_b = (t.clone() for t in step())
        ops.set_math_mode(ops.MATH_FP32)
        em = torch.expm1(mix)
        rel = lambda x, y: float(((x - y).abs().sum() / y.abs().sum()).item())  # noqa: E731
        other_mode = {
            "math": other, "value": round(world * args.batch * o_steps / o_elapsed, 1), "unit": "spectrograms/s", "steps": o_steps,
            "ms_per_step": round(1e3 * o_elapsed / o_steps, 3),
            "roofline": {k: o_roof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "kernel_ms_per_step", "dominant_instantiation")} if o_roof else None,
        }
        parity = {"what": "rel-L1 of the bf16x3 result against the fp32-MFMA result on the benchmark batch (contract: 1e-3 vs the reference)",
                  "pred_bin": rel(m_b * em, m_a * em), "pred_mono": rel(mono_b, mono_a)}
        # BASELINE config 2's literal dtype, a REPORTED mode (never `value`): one bf16 product per product (the hi halves of the same
        # split32 tensors: include/m2h.h M2H_MATH_BF16), with its distance from the fp32 result and whether that holds the contract
        b_elapsed, _, _ = timed_run("bf16", o_steps, 1, False)
        ops.set_math_mode(ops.MATH_BF16)
        m_c, mono_c = (t.clone() for t in step())
        ops.set_math_mode(ops.MATH_FP32)
        e_bin, e_mono = rel(m_c * em, m_a * em), rel(mono_c, mono_a)
        gflop = 0.4226 * (args.tm / 32.0) * args.batch * world
        bf16_mode = {
            "math": "bf16 (single product: hi*hi of the bf16 hi halves, fp32 accumulate; tensors stay split32, so this engine still moves both halves)",
            "value": round(world * args.batch * o_steps / b_elapsed, 1), "unit": "spectrograms/s", "steps": o_steps,
            "ms_per_step": round(1e3 * b_elapsed / o_steps, 3),
            "rel_l1_vs_fp32": {"pred_bin": e_bin, "pred_mono": e_mono}, "contract": 1e-3,
            "within_contract": bool(e_bin <= 1e-3 and e_mono <= 1e-3),
            "roofline": {"bound": "mfma", "achieved": round(gflop * o_steps / b_elapsed / 1e3, 2), "peak": PEAK_BF16, "unit": "TFLOP/s",
                         "frac": round(gflop * o_steps / b_elapsed / 1e3 / PEAK_BF16, 4)},
            "note": "reported mode only: the headline `value` is the bf16x3 arithmetic, which holds the fp32 contract by two orders of magnitude",
        }
        del m_a, m_b, mono_a, mono_b, m_c, mono_c, em
    ops.set_math_mode(ops.MATH_FP32)

    # the host-core baselines are single-GPU-run figures (rank 0, N = 1); the pair's comes first: its probe picks the thread count
    with_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    cpu = cpu_baseline(sd, args.tm, args.cpu_seconds) if with_cpu else None
    ddppo = run_ddppo(args, dev, rank, world, dist, with_cpu=with_cpu) if (args.full and args.ddppo_cycles > 0) else None
    ddppo_far = run_ddppo(args, dev, rank, world, dist, far_target=True) if (args.full and args.ddppo_cycles > 0 and not args.no_far_target) else None
    ptrain = run_passive_train(args, dev, rank, with_cpu=with_cpu) if (args.full and args.train_steps > 0) else None
    feeder = run_feeder(args, dev, rank, with_cpu=with_cpu) if (args.full and args.feeder_steps > 0) else None

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    # the clock the chip holds inside the dominant kernel family (the shared-patch engine), from a stamped run of the diagnostic library in
    # a child process, outside every timed region (N = 1 only): with it a box-to-box spread of ms_per_step can be told from a code change
    if roofline is not None:
        roofline["clock_ghz"], roofline["clock_probe"] = None, None
        if world == 1 and not args.no_clock_probe and args.math == "bf16x3":
            import subprocess
            try:
                torch.cuda.synchronize()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "clock_probe.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if not lines:
                    raise RuntimeError("tools/clock_probe.py printed no result (rc %d): %s" % (r.returncode, r.stderr[-240:]))
                probe = json.loads(lines[-1])
                roofline["clock_probe"] = probe
                if "layers" in probe:
                    dom = roofline["dominant_instantiation"]["name"]
                    same = [v for v in probe["layers"].values() if v["kernel"] == dom] or list(probe["layers"].values())
                    roofline["clock_ghz"] = round(sum(v["clock_ghz"] for v in same) / len(same), 3)
                    roofline["clock_ghz_what"] = ("in-kernel shader clock of %s (mean over the probe's layers on that kernel; per layer in clock_probe): "
                                                  "delta s_memtime / delta s_memrealtime around the k-loop, diagnostic build, outside the timed region; chip maximum 2.4" % dom)
            except Exception as exc:   # the probe is a diagnostic: its failure never fails the benchmark
                roofline["clock_probe"] = {"error": repr(exc)[:300]}

    value = world * args.batch * args.steps / elapsed
    line = {
        "metric": "passive_unet_pair_spectrograms_per_sec",
        "value": round(value, 1), "unit": "spectrograms/s",
        "n_gpus": world, "ranks_observed": ranks_observed, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("bf16x3 (fp32 tensors; each product = hi*hi + hi*lo + lo*hi of bf16 halves on the bf16 MFMA pipe, fp32 accumulate)"
                  if args.math == "bf16x3" else "f32"),
        "data": "synthetic",
        "config": {"workload": "passive U-Net separator pair forward (get_binSepMasks + convert_bin2mono, eval-BN), "
                               "batch %d/GPU of 512x%d binaural log-magnitude spectrograms, inputs resident in HBM" % (args.batch, args.tm),
                   "batch_per_gpu": args.batch, "n_freq": 512, "time_frames": args.tm, "parallelism": "dp%d (batch-sharded, no collective)" % world,
                   "weights": "synthetic (m2h.synthetic seed 1), reference architecture 33.47 M params",
                   "launch": ("two m2h_unet_fwd calls per step (22 kernels enqueued one by one)" if args.no_graph else
                              "HIP graph: the step's kernels (20 convs -- the first of each U-Net with the input slice fused in --, the split-K reduces of the deep stages) captured once per arithmetic mode, replayed every step (m2h.graphs)")},
        "roofline": roofline,
        "other_math_mode": other_mode,
        "other_math_modes": [m for m in (other_mode, bf16_mode) if m is not None],
        "math_mode_parity": parity,
        "ddppo": ddppo,
        "ddppo_far_target": ddppo_far,
        "passive_train": ptrain,
        "feeder": feeder,
        "cpu_baseline": cpu,
        "speedup_vs_cpu_baseline": round(value / cpu["value"], 1) if cpu else None,
        "layers": layers,
    }
    print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
