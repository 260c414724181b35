"""DD-PPO trainer on MI355X: the training cycle of audio_separation/rl/ppo/ppo_trainer.py (PPOTrainer, :40-1013) restated
around the m2h modules and the synthetic on-device environment.

Kept: the schedule (num_updates_per_cycle x (num_steps rollout + update_pol), then num_updates_per_cycle x update_sep;
:730-1011), _collect_rollout_step's data flow (:253-478), reward override incl. the extra reward at MAX_EPISODE_STEPS-2
(:385-405; its EFFECTIVE value, see _rollout_step_device), STFT-L2 bookkeeping (:407-420), linear LR / clip decay (:733-739,
:711-718), per-rank seeding (:609-611), the stats all-reduces and window-of-N statistics (:790-977), the checkpoint interval
(:1007-1009).  Pinned against the reference's own ``PPOTrainer.train`` run (tests/golden/trainer_*.npz, oracle/gen_trainer_golden.py;
tests/test_gpu_trainer_golden.py).  Changed in mechanism only:
  * no host sync inside the rollout step: the env consumes device actions, rewards/losses/statistics stay on the device
    (the reference does ~50 ``.item()``/``.cpu()`` per step);
  * the separator outputs for the *next* observation, which the reference computes for the reward (:358-373), are re-used as
    the *current* outputs of the following step (same frozen networks, same observation): half the U-Net passes, identical
    values; invalidated whenever acoustic_mem changes (after update_sep);
  * the same outputs are stored beside the observation in the separator storage, where update_sep reads them instead of
    re-running the frozen U-Nets over the whole buffer (the reference does that 24 x per cycle under no_grad, ppo.py:184-195);
  * checkpoints keep the reference format {"state_dict", "config"} (:223-238).
Out of scope: Habitat env construction, TensorBoard.
"""
import os
import time
import warnings
from collections import deque
from types import SimpleNamespace

import torch
from torch.optim.lr_scheduler import LambdaLR

from ... import graphs, ops
from ...common.rollout_storage import RolloutStoragePol, RolloutStorageSep
from ...common.utils import linear_decay
from ...envs.synthetic_env import SyntheticVecEnv
from .policy import Move2HearPolicy
from .ppo import DDPPO, PPO


def near_target_config(**over):
    """RL.PPO.* of config/train/nearTarget.yaml:17-56 (+ config/default.py:66-98 defaults) as a flat namespace."""
    c = dict(NUM_PROCESSES=14, NUM_UPDATES=16786, CHECKPOINT_INTERVAL=89, LOG_INTERVAL=50, SEED=0, EXTRA_RGB=False, EXTRA_DEPTH=True,
             MAX_EPISODE_STEPS=20, num_updates_per_cycle=6, hidden_size=512, value_loss_coef=0.5, bin_separation_loss_coef=1.0,
             mono_conversion_loss_coef=1.0, entropy_coef=0.20, lr_pol=1.0e-4, lr_sep=5.0e-4, clip_param=0.1, ppo_epoch=4,
             num_mini_batch=1, eps=1.0e-5, max_grad_norm=0.5, num_steps=20, use_gae=True, gamma=0.99, tau=0.95,
             use_linear_clip_decay=True, use_linear_lr_decay=True, sep_reward_weight=1.0, nav_reward_weight=0.0,
             extra_reward_multiplier=10.0, reward_window_size=50, use_ddppo=True, CHECKPOINT_FOLDER=None,
             switch_policy=False, time_thres_for_pol_switch=80, deterministic_eval=False,   # config/default.py:99-101
             ddppo_distrib_backend="NCCL", master_port=8738, master_addr="127.0.0.1",       # config/default.py:94-97
             short_rollout_threshold=1.0, sync_frac=0.6,  # nearTarget.yaml:58-59: at 1.0 the pre-emption of :775-781 never triggers (ddppo_utils.RolloutTracker)
             use_hip_graphs=True,       # build-side key: replay the rollout step and the update_pol epoch from HIP graphs (same kernels, same results)
             bucketed_grad_reduce=None,  # build-side key: None = when distributed, the policy gradient's all-reduce in two buckets, the first under the encoders' backward
             overlap_grad_reduce=None,  # build-side key: None = overlap the last all-reduce + step of an update when distributed
             pretrained_passive_separators_ckpt="", train_passive_separators=False,   # nearTarget.yaml:23-24 (accepted; see setup())
             rollout_math=None,         # build-side key: arithmetic of the rollout steps' conv / GEMM launches: None = the calling thread's mode (ops.set_math_mode);
             #                            "fp32" pins them to fp32 MFMA whatever the update phases compute in (the mixed-precision far-target leg: at 14
             #                            environments nothing is matrix-bound, and the one-launch / skinny kernels of that batch are fp32 kernels)
             overlap_update_tail=False,  # build-side key: the cycle's six update_sep on a second HIP stream beside the last update_pol (same bits,
             #                            tests/test_gpu_round4.py).  Off: measured +0.5 % only (profiles/r04_ddppo_tail_overlap_ab.txt) -- update_sep's
             #                            image-row kernels keep every CU's LDS occupied for their whole run, so the policy update's small
             #                            kernels wait for the gaps between them instead of running beside them
             sep_update_math=None,      # build-side key: arithmetic of update_sep's launches (AcousticMem over the 1680 stored samples: the one matrix-bound
             #                            phase of the cycle): None = the calling thread's mode; "bf16x3" = split bf16 products, fp32 accumulate (the
             #                            image-row kernels of csrc/conv_row3x3.hip / wgrad_row3x3.hip: ~6e-6 from the fp32 result, 1.36 -> 0.75 ms per epoch)
             action_sampling="fused")  # build-side key: "fused" = torch.multinomial's single draw with its Exp(1) noise made inside the heads kernel
    #                                     (Philox4x32-10, seed = SEED + rank offset, counter on the device: no generator launch in the step);
    #                                     "device" = the noise from torch's device generator; "cpu_generator" = from the CPU default generator:
    #                                     the reference PyTorch-CPU run's actions from the seed alone
    c["record_action_noise"] = False   # build-side key (fused sampling): keep every step's Exp(1) noise in actor_critic.last_action_noise -- the
    #                                     record tests/test_gpu_trainer_golden.py hands the CPU oracle's loop in place of its generator's draw
    c.update(over)
    return SimpleNamespace(**c)


def far_target_config(**over):
    """config/train/farTarget.yaml differs in reward weights and episode length only."""
    return near_target_config(**dict(dict(MAX_EPISODE_STEPS=80, sep_reward_weight=0.0, nav_reward_weight=1.0), **over))


class PPOTrainer:
    def __init__(self, config=None, device=None, world_rank=0, world_size=1, envs=None):
        """envs: optional environment object.  None = the synthetic on-device env; anything with ``reset() / step(actions)``
        returning device tensors as ``SyntheticVecEnv`` does -- e.g. ``HostVectorEnvAdapter`` around the reference's
        ``VectorEnvCustom`` (row N4) -- replaces it; without ``step_device`` the rollout step is enqueued kernel by kernel."""
        self.config = config if config is not None else near_target_config()
        self.device = device if device is not None else torch.device("cuda", 0)
        self.world_rank, self.world_size = world_rank, world_size
        self.actor_critic = None
        self.agent = None
        self.envs = envs
        self._next_cache = None
        self._mem_stale = False
        self._graph_state = None

    # ------------------------------------------------------------------ setup (reference :101-222, :542-577, :588-661)
    def setup(self, passive_state_dict=None):
        cfg = self.config
        seed = cfg.SEED + self.world_rank * cfg.NUM_PROCESSES
        torch.manual_seed(seed)
        if self.envs is None:
            self.envs = SyntheticVecEnv(cfg.NUM_PROCESSES, self.device, seed=seed, episode_len=cfg.MAX_EPISODE_STEPS)
        self.actor_critic = Move2HearPolicy(
            observation_space=self.envs.observation_spaces[0], action_space=self.envs.action_spaces[0], goal_sensor_uuid="spectrogram",
            hidden_size=cfg.hidden_size, extra_rgb=cfg.EXTRA_RGB, extra_depth=cfg.EXTRA_DEPTH, use_ddppo=cfg.use_ddppo,
            world_rank=self.world_rank)
        self.actor_critic.to(self.device)
        self.actor_critic.set_action_sampling(getattr(cfg, "action_sampling", "fused"), seed=0x5eed0000 + seed,
                                              record_noise_rows=cfg.NUM_PROCESSES if getattr(cfg, "record_action_noise", False) else None)
        cls = DDPPO if cfg.use_ddppo else PPO
        self.agent = cls(actor_critic=self.actor_critic, clip_param=cfg.clip_param, ppo_epoch=cfg.ppo_epoch,
                         num_mini_batch=cfg.num_mini_batch, value_loss_coef=cfg.value_loss_coef,
                         bin_separation_loss_coef=cfg.bin_separation_loss_coef, mono_conversion_loss_coef=cfg.mono_conversion_loss_coef,
                         entropy_coef=cfg.entropy_coef, lr_pol=cfg.lr_pol, lr_sep=cfg.lr_sep, eps=cfg.eps,
                         max_grad_norm=cfg.max_grad_norm,
                         freeze_passive_separators=not bool(getattr(cfg, "train_passive_separators", False)),   # :72-73 (stored, read nowhere)
                         overlap_grad_reduce=getattr(cfg, "overlap_grad_reduce", None),
                         bucketed_grad_reduce=getattr(cfg, "bucketed_grad_reduce", None),
                         use_hip_graphs=bool(getattr(cfg, "use_hip_graphs", False)))
        self.actor_critic.train()
        if passive_state_dict is not None:
            self.agent.load_pretrained_passive_separators(passive_state_dict)
        # the separators are frozen whatever RL.PPO.train_passive_separators says: the reference's train() always runs
        # _load_pretrained_passive_separators (:637-638), which freezes unconditionally (:557-577); the flag derived from the key
        # (:72-73) is stored by PPO and read nowhere.  Pinned by tests/golden/trainer_unfrozen.npz (the reference run with the key True).
        for name in ("binSep_enc", "binSep_dec", "bin2mono_enc", "bin2mono_dec"):
            m = getattr(self.actor_critic, name)
            m.eval()
            for p in m.parameters():
                p.requires_grad_(False)
        if cfg.use_ddppo:  # :639-640 -- at world size 1 too: DDPPO normalises advantages with the distributed (biased) variance
            self.agent.init_distributed(find_unused_params=True)
        N = self.envs.num_envs
        space = self.envs.observation_spaces[0]
        self.rollouts_pol = RolloutStoragePol(cfg.num_steps, N, space, cfg.hidden_size)
        self.rollouts_sep = RolloutStorageSep(cfg.num_steps * cfg.num_updates_per_cycle, N, space)
        # nearTarget/farTarget use one mini-batch: the update batch is the whole storage, read in place (rollout_storage.py)
        self.rollouts_pol.full_batch_views = True
        self.rollouts_sep.full_batch_views = True
        self.rollouts_pol.to(self.device)
        self.rollouts_sep.to(self.device)
        # the frozen separators' outputs of every stored observation are kept beside it (the rollout step computes them anyway), so
        # update_sep reads them instead of re-running the U-Nets over its 1 680-sample buffer (result-preserving: same networks, same
        # observations; module docstring)
        self.rollouts_sep.enable_separator_outputs()
        batch = self.envs.reset()
        for sensor in self.rollouts_pol.observations:
            self.rollouts_pol.observations[sensor][0].copy_(batch[sensor])
            self.rollouts_sep.observations[sensor][0].copy_(batch[sensor])
        self.rollouts_sep.touch()   # (a direct row write: the caches keyed on the storage's generation must see it)
        z = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
        self.stats = SimpleNamespace(
            episode_rewards=z(N, 1), episode_counts=z(N, 1), episode_steps=z(N, 1), episode_dist_probs=z(N, 3),
            episode_bin_losses_allSteps=z(N, 1), episode_mono_losses_lastStep=z(N, 1), episode_mono_losses_allSteps=z(N, 1),
            episode_monoFromMem_losses_lastStep=z(N, 1), episode_monoFromMem_losses_allSteps=z(N, 1), episode_ndgs=z(N, 1),
            episode_dgs=z(N, 1), current_episode_reward=z(N, 1), current_episode_step=z(N, 1), current_episode_dist_probs=z(N, 3),
            current_episode_bin_losses=z(N, 1), current_episode_mono_losses=z(N, 1), current_episode_monoFromMem_losses=z(N, 1))
        self._episode_step_host = 0
        self._stats_scratch = ops.step_stats_scratch(N, self.device) if self.device.type == "cuda" else None   # (one launch at a time per trainer)
        # the reference steps the LR schedulers at the START of each sub-update (:733-735, :981-982); torch warns about that order
        warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step\\(\\)` before `optimizer.step\\(\\)`")
        self.lr_scheduler_pol = LambdaLR(self.agent.optimizer_pol, lr_lambda=lambda x: linear_decay(x, cfg.NUM_UPDATES))
        self.lr_scheduler_sep = LambdaLR(self.agent.optimizer_sep, lr_lambda=lambda x: linear_decay(x, cfg.NUM_UPDATES))
        # straggler pre-emption (:597-600, :769-782): the "rollout_tracker/num_done" counter in the job's store; read only when
        # short_rollout_threshold < 1 lets a rollout end early
        from . import ddppo_utils
        # (at the shipped threshold 1.0 the counter can never be read -- `step >= num_steps` does not occur inside the loop -- so its store
        # traffic, two TCP round trips per rollout and rank, is not made either)
        self.rollout_tracker = (ddppo_utils.RolloutTracker(self.world_size, self.world_rank)
                                if cfg.use_ddppo and float(getattr(cfg, "short_rollout_threshold", 1.0)) < 1.0 else None)
        self.count_steps = 0
        self.num_updates_done = 0
        self.num_sep_updates_done = 0
        self.count_checkpoints = 0
        self.windows = {}      # window-of-N statistics (:699-709): name -> deque of summed-over-ranks [N,*] tensors
        self.scalars = []      # (count_steps, {tag: value}) per policy update: what the reference hands its TensorboardWriter

    # ------------------------------------------------------------------ rollout step (reference :253-478)
    def _separate(self, obs):
        ac = self.actor_critic
        pm = ac.get_binSepMasks(obs)
        mono = ac.convert_bin2mono(pm, mixed_audio=obs["mixed_bin_audio_mag"])
        return pm, mono

    def _collect_rollout_step(self):
        """One environment step for all envs (reference :253-478).  With ``use_hip_graphs`` the step is replayed from a HIP
        graph whenever the previous step left its next-observation separator outputs behind (every step but the first after
        update_sep); otherwise it is enqueued kernel by kernel."""
        cfg = self.config
        rm = getattr(cfg, "rollout_math", None)
        if rm is not None and ops.math_mode() != {"fp32": ops.MATH_FP32, "bf16x3": ops.MATH_BF16X3}[rm]:
            with ops.math_scope({"fp32": ops.MATH_FP32, "bf16x3": ops.MATH_BF16X3}[rm]):   # (graphs are keyed on the mode they were captured in)
                return self._collect_rollout_step()
        override = cfg.sep_reward_weight == 1.0 and cfg.nav_reward_weight == 0.0
        # :395 reads env 0's step count (current_episode_step[0].item(): a host sync); it is known on the host here
        extra = override and self._episode_step_host == cfg.MAX_EPISODE_STEPS - 2
        on_device = hasattr(self.envs, "step_device")  # host-side envs (the real simulator) report `done` themselves
        done = self.envs.t + 1 >= self.envs.episode_len if on_device else None
        if self._mem_stale and self._next_cache is not None:
            ro = self.rollouts_pol   # what the cache-less step computes from the same operands (_rollout_step_device, cache is None)
            with torch.no_grad():
                self._next_cache[2].copy_(self.actor_critic.get_monoFromMem_masked(self._next_cache[1], ro.prev_pred_monoFromMem[ro.step], ro.masks[ro.step]))
        self._mem_stale = False
        if on_device and self._graphs_enabled() and self._next_cache is not None:
            self._graph_step(extra, done)
            self.rollouts_pol.advance()  # the replayed inserts address their rows on the device
            self.rollouts_sep.advance(with_preds=True)
        else:
            with torch.no_grad():
                self._next_cache = self._rollout_step_device(self._next_cache, None, extra, done)
        # host-side counters
        if on_device:
            self.envs.t = 0 if done else self.envs.t + 1
            self._episode_step_host = 0 if done else self._episode_step_host + 1
        else:  # the adapter has the step's `dones` on the host already (it built the not-done masks from them)
            self._episode_step_host = 0 if self.envs.last_dones[0] else self._episode_step_host + 1
        return self.envs.num_envs

    def _rollout_step_device(self, cache, at, extra, done):
        """The device work of one rollout step.  With ``at`` it changes no host-side state, so it can be captured once and
        replayed (without ``at`` the storages' inserts advance their host step counters, as in the reference).
        cache: (pred_binSepMasks, pred_mono, pred_monoFromMem) of the current observation left by the previous step, or None.
        at: None = rows of the storages addressed by their host step counters (views); HIP-graph capture passes the device
        index tensor [ro_step, ro_step + 1, rs_step + 1] (rows then move through m2h_rows_copy).  extra / done: the two host-known schedule flags (extra reward at
        MAX_EPISODE_STEPS - 2, :395-405; lockstep episode end).  Returns the next step's cache."""
        cfg, ac, ro, rs, st = self.config, self.actor_critic, self.rollouts_pol, self.rollouts_sep, self.stats
        L = 512 * 32
        if at is None:
            row = lambda t: t[ro.step]  # noqa: E731
            step_observation = {k: row(v) for k, v in ro.observations.items()}
            step_masks, step_h = row(ro.masks), row(ro.recurrent_hidden_states_pol)
        else:  # rows addressed by the device-resident step index: one batched copy into this graph's own buffers
            src = dict(ro.observations, _masks=ro.masks, _h=ro.recurrent_hidden_states_pol)
            got = {k: torch.empty_like(v[0]) for k, v in src.items()}
            ops.rows_copy([(src[k], got[k], 0, -1) for k in src], at)
            step_masks, step_h = got.pop("_masks"), got.pop("_h")
            step_observation = got
            row = None  # (the previous memory is read only without a cache, which a captured step always has)
        if cache is not None:
            pred_binSepMasks, pred_mono, pred_monoFromMem = cache  # computed for the reward of the previous step
        else:
            pred_binSepMasks, pred_mono = self._separate(step_observation)
            pred_monoFromMem = ac.get_monoFromMem_masked(pred_mono, row(ro.prev_pred_monoFromMem), step_masks)
            rs.store_separator_outputs(rs.step, pred_binSepMasks, pred_mono)   # (the same observation sits in row rs.step of that storage)
        values, actions, actions_log_probs, recurrent_hidden_states_pol, distribution_probs = ac.act(
            step_observation, step_h, step_masks, pred_binSepMasks=pred_binSepMasks,
            pred_mono=pred_mono, pred_monoFromMem=pred_monoFromMem)
        # device in, device out; a host-side env (done is None) pays its device<->host round trip inside step()
        batch, rewards, masks, infos = self.envs.step_device(actions, done) if done is not None else self.envs.step(actions)
        # next-step predictions, needed for the reward of the present step (:358-373)
        next_pred_binSepMasks, next_pred_mono = self._separate(batch)
        next_pred_monoFromMem = ac.get_monoFromMem_masked(next_pred_mono, pred_monoFromMem, masks)
        # rewards (:385-405), STFT-L2 bookkeeping (:407-420) and the per-episode statistics (:421-455): one launch
        # (ops.rollout_step_stats).  On the extra-reward step the reference's override_rewards writes into the list it is given and
        # returns that same list (env_utils.py:692-706), so the "extra" call (:396-402) overwrites the quality-improvement rewards
        # and ``np.array(rewards) + np.array(rewards_extra)`` (:405) adds the list to itself: 2 x multiplier x util(next).
        # Pinned by tests/golden/trainer_near.npz (the reference's own loop).
        override = cfg.sep_reward_weight == 1.0 and cfg.nav_reward_weight == 0.0
        rewards, _losses = ops.rollout_step_stats(
            st, next_pred_monoFromMem, batch["gt_mono_comps"], pred_monoFromMem, step_observation["gt_mono_comps"], pred_binSepMasks,
            step_observation["mixed_bin_audio_mag"], step_observation["gt_bin_comps"], pred_mono, masks, distribution_probs,
            env_rewards=rewards, ndgs=infos.get("normalized_geo_distance_to_target_audio_source"),
            dgs=infos.get("geo_distance_to_target_audio_source"), override=override, extra=extra,
            extra_mult=2.0 * cfg.extra_reward_multiplier, scratch=self._stats_scratch)
        pol_args = (batch, recurrent_hidden_states_pol, actions, actions_log_probs, values, rewards, masks)
        pol_kw = dict(pred_binSepMasks=pred_binSepMasks, pred_mono=pred_mono, pred_monoFromMem=pred_monoFromMem)
        if at is None:
            ro.insert(*pol_args, **pol_kw)
            rs.insert(batch, masks, pred_monoFromMem=pred_monoFromMem, pred_binSepMasks=next_pred_binSepMasks, pred_mono=next_pred_mono)
        else:
            ops.rows_copy(ro.insert_items((0, 1), *pol_args, **pol_kw) +
                          rs.insert_items(2, batch, masks, pred_monoFromMem=pred_monoFromMem, pred_binSepMasks=next_pred_binSepMasks,
                                          pred_mono=next_pred_mono), at)
            # hand the next-observation separator outputs over to the following step's static buffers: one batched copy, AFTER the
            # inserts above have read those buffers (they hold this step's outputs)
            nxt = (next_pred_binSepMasks, next_pred_mono, next_pred_monoFromMem)
            ops.rows_copy([(src.contiguous(), dst, -1, -1) for src, dst in zip(nxt, cache)], at)
            return cache
        return next_pred_binSepMasks, next_pred_mono, next_pred_monoFromMem

    # ------------------------------------------------------------------ HIP-graph replay of the rollout step
    def _graphs_enabled(self):
        return bool(getattr(self.config, "use_hip_graphs", False)) and not ops.timing_enabled()

    def _graph_step(self, extra, done):
        """The rollout step is ~150 small launches behind ~2 ms of Python; its device work depends on the host only through
        (extra, done), so one HIP graph per flag pair is captured on first use and replayed afterwards.  The graph reads the
        step's rows of the storages through device-resident indices (advanced inside the graph), the previous step's
        separator outputs from three static buffers, and the policy / acoustic-memory weights by address: parameters live in
        FlatAdam's flat buffers and packed copies are refreshed in place (functional.refresh_pack_memos) before a replay."""
        from ... import functional as MF
        ro, rs = self.rollouts_pol, self.rollouts_sep
        gs = self._graph_state
        if gs is None:
            dev = self.device
            gs = self._graph_state = SimpleNamespace(
                graphs={}, pool=None, where=None, idx=torch.zeros(3, dtype=torch.int64, device=dev), expect=None, epoch=None, noise_rows=None,
                sampling=self.actor_critic.sampling_key(),
                cache=tuple(torch.empty_like(t) for t in self._next_cache))
        if self._next_cache[0] is not gs.cache[0]:  # the previous step ran outside the graphs: hand its outputs over
            for dst, src in zip(gs.cache, self._next_cache):
                dst.copy_(src)
            self._next_cache = gs.cache
        if gs.expect != (ro.step, rs.step):  # device indices out of step with the host counters (eager steps in between)
            for j, v in enumerate((ro.step, ro.step + 1, rs.step + 1)):
                gs.idx[j:j + 1].fill_(v)
        if gs.epoch != MF.param_epoch():
            self.agent.optimizer_pol.build()  # parameters move into the flat buffers once; the graphs hold their addresses
            self.agent.optimizer_sep.build()
            self.actor_critic._fence("pol")
            self.actor_critic._fence("mem")
            MF.refresh_pack_memos()
            gs.epoch = MF.param_epoch()
            where = (ops.math_mode(),) + tuple(p.data_ptr() for p in self.actor_critic.parameters())
            if where != gs.where:  # a parameter was re-allocated (first build, .to(), ...): captured addresses are stale
                gs.graphs.clear()
                gs.where = where
        if gs.sampling != self.actor_critic.sampling_key():   # set_action_sampling since the capture: another draw, or its state elsewhere
            gs.graphs.clear()
            gs.sampling = self.actor_critic.sampling_key()
        key = (bool(extra), bool(done), ops.math_mode())   # (a graph is the kernels of ONE arithmetic: a mode change captures anew)
        g = gs.graphs.get(key)
        if g is None:
            self.actor_critic.prepare_action_sampling(self.envs.num_envs)   # (pinned / static buffers cannot be made inside a capture)
            g = torch.cuda.CUDAGraph()
            g.register_generator_state(self.envs.generator)
            with torch.no_grad(), graphs.capture(g, pool=gs.pool):
                self._rollout_step_device(gs.cache, gs.idx, extra, done)   # (leaves the next step's separator outputs in gs.cache)
                rng = self.actor_critic._rng_state    # "fused" sampling: the step's draws consumed NUM_PROCESSES x actions counters
                ops.step_index_advance(gs.idx, ro.num_steps, rs.num_steps, rng=rng,   # ro_step <- (ro_step + 1) % T, rs_step likewise
                                       rng_inc=self.envs.num_envs * self.actor_critic.dim_actions if rng is not None else 0)
            if gs.pool is None:
                gs.pool = g.pool()
            gs.graphs[key] = g
            gs.noise_rows = self.envs.num_envs     # the captured act() reads the static [rows, actions] noise buffer of THIS row count
        if gs.noise_rows != self.envs.num_envs:
            raise RuntimeError("m2h PPOTrainer: the rollout graph was captured for %d envs, the env now has %d" % (gs.noise_rows, self.envs.num_envs))
        # cpu_generator sampling: a graph that contains sample() must be replayed through here -- the noise of THIS step is drawn on
        # the host and staged into the buffer the graph reads before every replay (a bare g.replay() would re-use the last step's)
        self.actor_critic.stage_action_noise(self.envs.num_envs)
        graphs.replay(g)
        gs.expect = ((ro.step + 1) % ro.num_steps, (rs.step + 1) % rs.num_steps)

    # ------------------------------------------------------------------ updates (reference :480-541)
    def _update_pol(self, as_tensor=False):
        cfg, ro = self.config, self.rollouts_pol
        with torch.no_grad():
            last_observation = {k: v[-1] for k, v in ro.observations.items()}
            next_value = self.actor_critic.get_value(
                last_observation, ro.recurrent_hidden_states_pol[-1], ro.masks[-1], pred_binSepMasks=ro.pred_binSepMasks[-1],
                pred_mono=ro.pred_mono[-1], pred_monoFromMem=ro.prev_pred_monoFromMem[-1]).detach()
        ro.compute_returns(next_value, cfg.use_gae, cfg.gamma, cfg.tau)
        out = self.agent.update_pol(ro, as_tensor=as_tensor)
        ro.after_update()
        return out

    _MATH = {"fp32": ops.MATH_FP32, "bf16x3": ops.MATH_BF16X3}

    def _update_sep(self, as_tensor=False):
        sm = getattr(self.config, "sep_update_math", None)
        if sm is not None and ops.math_mode() != self._MATH[sm]:
            with ops.math_scope(self._MATH[sm]):    # (autograd Functions carry the forward's mode into their backward)
                return self._update_sep(as_tensor)
        out = self.agent.update_sep(self.rollouts_sep, as_tensor=as_tensor)
        self.rollouts_sep.after_update()
        # acoustic_mem changed: the cached memory output of the current observation is stale -- and only that: the separators are frozen
        # (setup()), their two cached outputs of the same observation still hold.  The next rollout step recomputes the memory's (one
        # launch) and replays its graph; dropping the whole cache made that step the cycle's one kernel-by-kernel step (1.2 ms against 0.46)
        self._mem_stale = self._next_cache is not None
        return out

    def train_cycle(self, log_stats=False, checkpoint=False, phase_events=None):
        """One cycle of the reference schedule (:730-1011): returns a dict of timings and losses.
        phase_events: optional list; gets one (phase, start event, end event) triple per rollout / update_pol / update_sep of the
        cycle, recorded on the compute stream (bench.py's per-phase breakdown; deferred optimizer steps run on the side stream and
        show up in ddppo_utils.collective_log instead).
        log_stats: after every policy update compute the window-of-N statistics the reference writes to TensorBoard (:790-977;
        one stats all-reduce + one small device->host read per update) and append them to ``self.scalars``.
        checkpoint: save ``ckpt.<k>.pth`` whenever the separator update number is a multiple of CHECKPOINT_INTERVAL (:1007-1009)."""
        cfg = self.config
        t0 = time.perf_counter()
        steps = 0
        pol_losses, sep_losses, tail, sep_pending = None, None, False, None
        for _sub in range(cfg.num_updates_per_cycle):
            if cfg.use_linear_lr_decay:
                self.lr_scheduler_pol.step()
            if cfg.use_linear_clip_decay:
                self.agent.clip_param = cfg.clip_param * linear_decay(self.num_updates_done, cfg.NUM_UPDATES)
            sub_steps = 0
            e0 = self._mark(phase_events)
            for _step in range(cfg.num_steps):
                sub_steps += self._collect_rollout_step()
                if self.rollout_tracker is not None and self.rollout_tracker.should_preempt(
                        _step, cfg.num_steps, getattr(cfg, "short_rollout_threshold", 1.0), getattr(cfg, "sync_frac", 0.6)):
                    break      # :775-780: enough of the other ranks are waiting at the update
            if self.rollout_tracker is not None:
                self.rollout_tracker.rollout_done()        # :781-782
            steps += sub_steps
            e1 = self._mark(phase_events)
            tail = _sub == cfg.num_updates_per_cycle - 1 and self._tail_overlap(checkpoint)
            if tail:
                sep_pending = self._enqueue_separator_updates(phase_events)
            # (without the window statistics nothing on the host needs the losses before the cycle ends: they stay on the device, and the
            # next rollout's steps are enqueued under this update's last optimizer step)
            pol_losses = self._update_pol(as_tensor=self.device.type == "cuda" and not log_stats)
            if phase_events is not None:
                phase_events += [("rollout", e0, e1), ("update_pol", e1, self._mark(phase_events))]
            self.num_updates_done += 1
            if log_stats:
                self._log_window_stats(pol_losses, sub_steps)
            if self.rollout_tracker is not None:
                self.rollout_tracker.reset()               # :862-863 (world rank 0, behind the update's statistics all-reduce)
        if tail:
            torch.cuda.current_stream(self.device).wait_stream(self._tail_stream)
            sep_losses = tuple(sep_pending[-1].tolist())
        sep_dev = None
        for _sub in range(0 if tail else cfg.num_updates_per_cycle):
            if cfg.use_linear_lr_decay:
                self.lr_scheduler_sep.step()
            e0 = self._mark(phase_events)
            # the losses stay on the device until the cycle's last update has been enqueued: read as floats after every update (a host
            # synchronisation each) the next update's preparation -- storage roll-over, the memory's sliced input: ~350 us of launches
            # paced by the host -- could not be enqueued under the running epochs (rocprofv3: 470 us between two updates' epochs)
            sep_dev = self._update_sep(as_tensor=self.device.type == "cuda")
            if phase_events is not None:
                phase_events.append(("update_sep", e0, self._mark(phase_events)))
            if checkpoint and self.world_rank == 0 and self.num_sep_updates_done % cfg.CHECKPOINT_INTERVAL == 0 and cfg.CHECKPOINT_FOLDER:
                self.save_checkpoint("ckpt.%d.pth" % self.count_checkpoints)
                self.count_checkpoints += 1
            self.num_sep_updates_done += 1
        if sep_dev is not None:
            sep_losses = tuple(sep_dev.tolist()) if torch.is_tensor(sep_dev) else sep_dev
        if torch.is_tensor(pol_losses):
            pol_losses = tuple(pol_losses.tolist())
        if not log_stats:
            self.count_steps += steps
        return {"env_steps": steps, "seconds": time.perf_counter() - t0, "pol_losses": pol_losses, "sep_losses": sep_losses}

    # ------------------------------------------------------------------ the cycle's tail: update_pol #6 beside the six update_sep
    # After the last rollout of a cycle nothing links the last policy update (policy network + heads, policy storage, "pol" optimizer)
    # to the separator updates (AcousticMem, separator storage, "mem" optimizer): the reference runs them one after the other
    # (:730-1011), here the six update_sep are enqueued on a second HIP stream -- no host synchronisation inside: their losses stay on
    # the device until the join -- and the policy update runs beside them on the compute stream.  Same kernels on the same data in the
    # same per-stream order: the same bits (tests/test_gpu_round4.py).  Opt-in (overlap_update_tail): measured, the policy update's small
    # launches find no room beside update_sep's image-row kernels (2 x 67 KB of LDS per CU for a launch's whole run) and the cycle gains
    # 0.5 % (12 560-12 670 -> 12 630-12 720 env-steps/s).  The CPU generator's randperm draws of the two phases swap places;
    # with full-batch views (one mini-batch) their values are never used and each advances the generator by the same amount.
    def _tail_overlap(self, checkpoint):
        cfg = self.config
        return (bool(getattr(cfg, "overlap_update_tail", False)) and self.device.type == "cuda" and not checkpoint and cfg.num_mini_batch == 1
                and getattr(self.rollouts_sep, "full_batch_views", False) and getattr(self.rollouts_pol, "full_batch_views", False)
                and not ops.timing_enabled())

    _tail_stream = None

    def _enqueue_separator_updates(self, phase_events):
        cfg = self.config
        main = torch.cuda.current_stream(self.device)
        if self._tail_stream is None:
            self._tail_stream = torch.cuda.Stream(self.device)
        # the second stream starts where the compute stream stands; the host waits for that point first, so that the stream's first
        # packet is not parked behind the rollout's replays (a parked cross-queue wait slows the running queue: m2h/graphs.py)
        main.synchronize()
        out = []
        with torch.cuda.stream(self._tail_stream):
            for _sub in range(cfg.num_updates_per_cycle):
                if cfg.use_linear_lr_decay:
                    self.lr_scheduler_sep.step()
                e0 = self._mark(phase_events)
                out.append(self._update_sep(as_tensor=True))
                if phase_events is not None:
                    phase_events.append(("update_sep", e0, self._mark(phase_events)))
                self.num_sep_updates_done += 1
        return out

    def _mark(self, sink):
        if sink is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        ev.m2h_kernels = graphs.launch_total()   # (host-side count at this point of the enqueue order: bench.py's launches per phase)
        return ev

    _WINDOW_KEYS = (("count", "episode_counts"), ("reward", "episode_rewards"), ("step", "episode_steps"), ("dist_probs", "episode_dist_probs"),
                    ("avg_bin_loss_allSteps", "episode_bin_losses_allSteps"), ("mono_loss_lastStep", "episode_mono_losses_lastStep"),
                    ("mono_loss_allSteps", "episode_mono_losses_allSteps"), ("monoFromMem_loss_lastStep", "episode_monoFromMem_losses_lastStep"),
                    ("monoFromMem_loss_allSteps", "episode_monoFromMem_losses_allSteps"),
                    ("normalized_geo_distance_to_target_audio_source", "episode_ndgs"), ("geo_distance_to_target_audio_source", "episode_dgs"))
    _SCALAR_TAGS = (("Environment/Reward", "reward"), ("Environment/Episode_length", "step"),
                    ("Environment/STFT_L2_loss/mono_lastStep", "mono_loss_lastStep"), ("Environment/STFT_L2_loss/mono_avgAllSteps", "mono_loss_allSteps"),
                    ("Environment/STFT_L2_loss/monoFromMem_lastStep", "monoFromMem_loss_lastStep"),
                    ("Environment/STFT_L2_loss/monoFromMem_avgAllSteps", "monoFromMem_loss_allSteps"),
                    ("Environment/Normalized_geo_distance_to_target_audio_source", "normalized_geo_distance_to_target_audio_source"),
                    ("Environment/Geo_distance_to_target_audio_source", "geo_distance_to_target_audio_source"))

    def _log_window_stats(self, pol_losses, steps_delta):
        """The logging of one policy update (:790-977).  Every per-env statistic is summed over ranks (the reference stacks them
        and all-reduces, :839-843; here they travel as ONE tensor together with the losses and the step count), pushed into a
        window of ``reward_window_size`` updates, and the logged value is (newest - oldest) summed over envs divided by the
        window's episode count (at least 1)."""
        from . import ddppo_utils
        cfg, st = self.config, self.stats
        N = self.envs.num_envs
        names = [n for _k, n in self._WINDOW_KEYS]
        cols = torch.cat([getattr(st, n) for n in names], dim=1)                              # [N, 10 + A]
        tail = torch.zeros(N, 4, device=self.device)
        tail[0] = torch.tensor(list(pol_losses) + [float(steps_delta)], device=self.device)   # :861-866
        packed = ddppo_utils.all_reduce_stats(torch.cat([cols, tail], dim=1)).cpu()           # the update's one extra host read
        v_loss, a_loss, ent, d_steps = (packed[0, -4:] / torch.tensor([self.world_size] * 3 + [1.0])).tolist()
        self.count_steps += d_steps
        deltas, off = {}, 0
        for key, name in self._WINDOW_KEYS:
            w = getattr(st, name).shape[1]
            cur = packed[:, off:off + w].clone()
            off += w
            win = self.windows.setdefault(key, deque(maxlen=cfg.reward_window_size))
            win.append(cur)
            d = (win[-1] - win[0]) if len(win) > 1 else win[0]
            deltas[key] = d.sum(dim=0) if key == "dist_probs" else d.sum().item()
        deltas["count"] = max(deltas["count"], 1.0)
        sc = {tag: deltas[key] / deltas["count"] for tag, key in self._SCALAR_TAGS}
        for i in range(deltas["dist_probs"].numel()):
            sc["Policy/Action_prob_%d" % i] = (deltas["dist_probs"] / deltas["count"])[i].item()
        sc.update({"Policy/Value_Loss": v_loss, "Policy/Action_Loss": a_loss, "Policy/Entropy": ent,
                   "Policy/Learning_Rate": self.lr_scheduler_pol.get_last_lr()[0]})
        self.scalars.append((self.count_steps, sc))
        return sc

    def all_reduce_stats(self):
        """The per-update statistics all-reduces of :790-860, fused into one small collective."""
        st = self.stats
        t = torch.cat([st.episode_rewards, st.episode_counts, st.episode_steps, st.episode_bin_losses_allSteps,
                       st.episode_mono_losses_lastStep, st.episode_monoFromMem_losses_lastStep], dim=1).sum(0)
        from . import ddppo_utils
        return ddppo_utils.all_reduce_stats(t)

    def save_checkpoint(self, file_name):
        ckpt = {"state_dict": {"actor_critic." + k: v for k, v in self.actor_critic.state_dict().items()}, "config": dict(vars(self.config))}
        # the file keeps the reference's two keys (:223-238); the fused sampler's [seed, counter] rides in the config (a build-side key like
        # action_sampling itself), so a run that continues from this file draws on from here instead of replaying the first steps' noise
        sampler = self.actor_critic.sampler_state()
        if sampler is not None:
            ckpt["config"]["m2h_sampler_state"] = sampler
        os.makedirs(self.config.CHECKPOINT_FOLDER, exist_ok=True)
        torch.save(ckpt, os.path.join(self.config.CHECKPOINT_FOLDER, file_name))

    def load_checkpoint(self, checkpoint_path, *args, **kwargs):
        """torch.load of a {"state_dict", "config"} checkpoint (reference :240-251); returns the dict."""
        kwargs.setdefault("map_location", "cpu")
        kwargs.setdefault("weights_only", False)
        return torch.load(checkpoint_path, *args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, sampler_state=None):
        """Loads agent weights saved by this trainer or by the reference (keys rooted at "actor_critic.").
        sampler_state: a checkpoint's config["m2h_sampler_state"] ([seed, counter] of the fused action sampler), restored in place."""
        sd = {k[len("actor_critic."):]: v for k, v in state_dict.items() if k.startswith("actor_critic.")}
        if not sd:
            raise RuntimeError("checkpoint state_dict has no 'actor_critic.*' keys")
        self.agent.synchronize_updates()  # a deferred optimizer step may still be writing the parameters
        out = self.actor_critic.load_state_dict(sd, strict=strict)
        from ... import functional as MF
        MF.bump_param_epoch()  # packed-weight memos key on the optimizer epoch
        self._next_cache = None
        self.rollouts_sep.invalidate_separator_outputs()
        self._drop_graphs()    # the frozen separators' packed weights / folded-BN buffers are rebuilt at new addresses
        self.actor_critic.restore_sampler_state(sampler_state)
        return out

    def _drop_graphs(self):
        """Forget every captured HIP graph (rollout step, update_pol epoch, update_sep epoch): they hold device addresses of packed weights and
        of the arithmetic-mode-specific operand copies, which a weight load or ``ops.set_math_mode`` replaces."""
        self._graph_state = None
        if self.agent is not None:
            self.agent._pol_graph = None
            self.agent._sep_graph = None

    @staticmethod
    def save_switch_checkpoint(path, nav_checkpoint, qual_improv_checkpoint):
        """The far-target evaluation's two-policy checkpoint (scripts/farTarget_eval/copy_individualCkptsNCfgs_switchPolicyEval.ipynb):
        ``state_dict_nav`` / ``config_nav`` from the far-target (navigation) run, ``state_dict_qualImprov`` /
        ``config_qualImprov`` from the near-target (quality-improvement) run.  Arguments: checkpoint dicts or paths."""
        load = lambda c: c if isinstance(c, dict) else torch.load(c, map_location="cpu", weights_only=False)  # noqa: E731
        nav, qual = load(nav_checkpoint), load(qual_improv_checkpoint)
        torch.save({"state_dict_nav": nav["state_dict"], "config_nav": nav["config"],
                    "state_dict_qualImprov": qual["state_dict"], "config_qualImprov": qual["config"]}, path)

    def _policy_from_state_dict(self, state_dict):
        """A second eval-mode Move2HearPolicy (same construction as setup()) carrying a checkpoint's ``actor_critic.*`` weights."""
        cfg = self.config
        ac = Move2HearPolicy(observation_space=self.envs.observation_spaces[0], action_space=self.envs.action_spaces[0],
                             goal_sensor_uuid="spectrogram", hidden_size=cfg.hidden_size, extra_rgb=cfg.EXTRA_RGB, extra_depth=cfg.EXTRA_DEPTH,
                             use_ddppo=cfg.use_ddppo, world_rank=self.world_rank)
        sd = {k[len("actor_critic."):]: v for k, v in state_dict.items() if k.startswith("actor_critic.")}
        if not sd:
            raise RuntimeError("checkpoint state_dict has no 'actor_critic.*' keys")
        ac.load_state_dict(sd, strict=True)
        ac = ac.to(self.device).eval()
        ac.set_action_sampling(getattr(cfg, "action_sampling", "fused"), seed=0x5eed1000 + cfg.SEED + self.world_rank * cfg.NUM_PROCESSES)
        return ac

    def eval(self, num_episodes=None, checkpoint_path=None, waveform_metrics=("si_sdr",), deterministic=None,
             switch_checkpoint_path=None, time_thres_for_pol_switch=None, trace=None):
        """Evaluation loop of `_eval_checkpoint` (reference :1015-1551) on this trainer's vectorised env: eval-mode policy,
        deterministic or sampled actions (ppo_cfg.deterministic_eval), per-step STFT-L2 of the separated mono (:1369-1385),
        waveform metrics of the LAST step of each episode (:1400-1415) when the env provides `mixed_bin_audio_phase`, and the
        reference's aggregation (mean / std over episodes, :1484-1504).  Returns the aggregated-stats dict.
        switch_checkpoint_path: the far-target evaluation with TWO policies (RL.PPO.switch_policy, :1093-1130, :1231-1312): a file
        holding ``state_dict_nav`` and ``state_dict_qualImprov``; the navigation policy (with its own separators, memory and
        hidden state) acts for the first ``time_thres_for_pol_switch`` steps of an episode (config/default.py:101: 80), the
        quality-improvement policy afterwards; the memory is masked by the navigation policy's not-done flags throughout and the
        quality-improvement policy's flags start tracking the env only once it acts (:1348-1360).
        trace: optional list; gets one (actions, mono STFT-L2, monoFromMem STFT-L2) tuple of host tensors per step (tests).
        Pinned against the reference's own ``_eval_checkpoint`` run (tests/golden/trainer_eval.npz, one and two policies)."""
        import numpy as np
        from ...common import eval_metrics as EM
        cfg, ac = self.config, self.actor_critic
        if checkpoint_path is not None:
            ck = self.load_checkpoint(checkpoint_path)
            self.load_state_dict(ck["state_dict"])   # (evaluation draws from its own seed, as the reference's eval does: no sampler state)
        acs = None
        if switch_checkpoint_path is not None:
            ck = self.load_checkpoint(switch_checkpoint_path)
            if "state_dict_nav" not in ck or "state_dict_qualImprov" not in ck:
                raise RuntimeError("switch-policy checkpoint needs 'state_dict_nav' and 'state_dict_qualImprov' (save_switch_checkpoint)")
            acs = (self._policy_from_state_dict(ck["state_dict_nav"]), self._policy_from_state_dict(ck["state_dict_qualImprov"]))
            thres = int(time_thres_for_pol_switch if time_thres_for_pol_switch is not None else getattr(cfg, "time_thres_for_pol_switch", 80))
        training_flags = {m: m.training for m in ac.modules()}   # the frozen separators stay in eval mode inside a training policy (:557-577)
        ac.eval()
        N = self.envs.num_envs
        num_episodes = num_episodes or N
        deterministic = getattr(cfg, "deterministic_eval", False) if deterministic is None else deterministic
        had_phase = getattr(self.envs, "include_phase", None)
        if had_phase is not None:
            self.envs.include_phase = bool(waveform_metrics)
        obs = self.envs.reset()
        h = torch.zeros(ac.pol_net.num_recurrent_layers, N, cfg.hidden_size, device=self.device)
        not_done = torch.ones(N, 1, device=self.device)
        h_q, not_done_q, step_in_episode = torch.zeros_like(h), torch.ones(N, 1, device=self.device), 0  # switch-policy state
        prev_mem = torch.zeros(N, 512, 32, 1, device=self.device)
        per_ep = {k: [] for k in ("mono_loss_last_step", "mono_loss_all_steps", "monoFromMem_loss_last_step",
                                  "monoFromMem_loss_all_steps", "reward")}
        wave = {"mono": {m: [] for m in waveform_metrics}, "monoFromMem": {m: [] for m in waveform_metrics}}
        cur_mono, cur_mem, cur_rew, cur_steps = (torch.zeros(N, 1, device=self.device) for _ in range(4))
        done_eps = 0
        with torch.no_grad():
            while done_eps < num_episodes:
                qual = acs is not None and step_in_episode >= thres            # :1231-1240 (step count of env 0: lockstep episodes)
                pol = ac if acs is None else acs[1 if qual else 0]
                pm = pol.get_binSepMasks(obs)
                mono = pol.convert_bin2mono(pm, mixed_audio=obs["mixed_bin_audio_mag"])
                mem = pol.get_monoFromMem_masked(mono, prev_mem, not_done)      # the nav flags mask the memory in both phases (:1276-1281)
                if qual:
                    _v, actions, _lp, h_q, _probs = pol.act(obs, h_q, not_done_q, deterministic=deterministic, pred_binSepMasks=pm,
                                                            pred_mono=mono, pred_monoFromMem=mem)
                else:
                    _v, actions, _lp, h, _probs = pol.act(obs, h, not_done, deterministic=deterministic, pred_binSepMasks=pm, pred_mono=mono,
                                                          pred_monoFromMem=mem)
                _db, d_mono = EM.STFT_L2_distance(obs["mixed_bin_audio_mag"], pm, obs["gt_bin_comps"], mono, obs["gt_mono_comps"])
                d_mem = ops.stft_l2(mem, obs["gt_mono_comps"], 1)
                last_obs, last_mono, last_mem = obs, mono, mem
                if trace is not None:
                    trace.append((actions.cpu(), d_mono.cpu(), d_mem.cpu()))
                obs, rewards, not_done, _infos = self.envs.step(actions)
                if qual:
                    not_done_q = not_done                                        # :1354-1359
                cur_mono += d_mono
                cur_mem += d_mem
                cur_rew += rewards
                cur_steps += 1
                prev_mem = mem
                finished = (not_done.view(-1) == 0).nonzero().view(-1).tolist()  # host sync once per step, as the reference's loop
                step_in_episode = 0 if 0 in finished else step_in_episode + 1    # :1216 (env 0's step count)
                if finished:
                    wm = None
                    if waveform_metrics and "mixed_bin_audio_phase" in last_obs:
                        gm, gp = last_obs["gt_mono_comps"][..., 0:1], last_obs["gt_mono_comps"][..., 1:2]
                        wm = {k: EM.waveform_metrics(gm, gp, v, last_obs["mixed_bin_audio_mag"], last_obs["mixed_bin_audio_phase"]).cpu()
                              for k, v in (("mono", last_mono), ("monoFromMem", last_mem))}
                    for e in finished:
                        if done_eps >= num_episodes:
                            break
                        n = float(cur_steps[e])
                        per_ep["mono_loss_last_step"].append(float(d_mono[e]))
                        per_ep["mono_loss_all_steps"].append(float(cur_mono[e]) / n)
                        per_ep["monoFromMem_loss_last_step"].append(float(d_mem[e]))
                        per_ep["monoFromMem_loss_all_steps"].append(float(cur_mem[e]) / n)
                        per_ep["reward"].append(float(cur_rew[e]))
                        if wm is not None:
                            for k in wave:
                                for m in waveform_metrics:
                                    wave[k][m].append(float(wm[k][e, EM.METRIC_ORDER.index(m)]))
                        done_eps += 1
                    for t in (cur_mono, cur_mem, cur_rew, cur_steps):
                        t.mul_(not_done)
        for m, flag in training_flags.items():
            m.training = flag
        if had_phase is not None:
            self.envs.include_phase = had_phase
        self._next_cache = None
        agg = {k: {"mean": float(np.mean(v)), "std": float(np.std(v))} for k, v in per_ep.items()}
        for k in wave:
            for m, v in wave[k].items():
                if v:
                    agg["%s_%s" % (k, m)] = {"mean": float(np.mean(v)), "std": float(np.std(v))}
        agg["num_episodes"] = done_eps
        return agg

    def train(self, num_cycles=None, log_stats=True, checkpoint=True):
        """The reference's training loop (:730-1011): ``NUM_UPDATES / num_updates_per_cycle`` cycles (or ``num_cycles``), window
        statistics after every policy update, a checkpoint every CHECKPOINT_INTERVAL separator updates (rank 0)."""
        cfg = self.config
        total = int(cfg.NUM_UPDATES / cfg.num_updates_per_cycle)
        out = []
        for _ in range(total if num_cycles is None else min(int(num_cycles), total)):
            out.append(self.train_cycle(log_stats=log_stats, checkpoint=checkpoint))
        return out
