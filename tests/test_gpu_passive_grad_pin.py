"""GPU: the gradient of one whole passive training step as shipped (PassiveTrainer: HIP graph on, weight gradients on side branches of
the graph, FlatAdam) against float64 autograd of m2h_oracle.passive_losses (train-mode BatchNorm; binSep on its own loss, bin2mono on the
detached masks) from the same weights and batch, every parameter tensor on its own; and the deferred weight gradients' aliasing of their
FlatAdam slots.

The end-to-end training tests compare weights after Adam, whose first steps are +-lr per element (the gradient's sign); this one pins the
gradient's size.  Metric per tensor: relative L2 ||g - r|| / ||r|| and the least-squares scale <g, r> / <r, r>.

The fp32 step differs from fp64 by more than rounding: a ReLU / LeakyReLU whose argument is near 0 can take the other branch in fp32, and
the gradient there changes by a whole unit.  Such a flip in a decoder stage reaches every layer upstream of it in the backward pass and
none downstream.  Measured on an MI355X: at B 64, per-tensor relative L2 up to 3.8e-3 (bin2mono's bottleneck layers, whose gradients are
sums over 64 - 256 rows; 5e-4 in binSep; 1e-5 .. 3e-5 at the output stages), |scale - 1| up to 2.8e-4; at B 5, 7.4e-6 and 1.7e-6.  The
bounds (8e-3, 1e-3) sit about 2x and 4x above that; a tensor scaled by 0.99 fails both.  Value bugs at these shapes are pinned element by
element, flip-free, by tests/test_gpu_grad_routes.py."""
import numpy as np
import pytest
import torch

import m2h_oracle as O
from m2h import synthetic

pytestmark = pytest.mark.gpu

L2_BOUND = 8e-3
SCALE_BOUND = 1e-3


def _batch(B, seed, dev):
    mixed, tc = synthetic.make_passive_inputs(B, 32, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    gt_bin = torch.rand(B, 512, 32, 2, generator=gen) * 2
    gt_mono = torch.rand(B, 512, 32, 1, generator=gen) * 2
    return [torch.from_numpy(mixed).to(dev), gt_bin.to(dev), gt_mono.to(dev), torch.from_numpy(tc).to(dev)]


def _graphed_step(B):
    """Two train_batch calls (the first runs kernel by kernel and moves the weights; the second captures and replays the step's graph):
    (weights before the second call, its batch, the gradients it left in FlatAdam's flat buffer, aliasing failures)."""
    from m2h.pretrain.passive.passive_trainer import PassiveTrainer, passive_config
    dev = torch.device("cuda", 0)
    tr = PassiveTrainer(passive_config(BATCH_SIZE=B), dev)
    assert tr.config.use_hip_graphs and tr.config.wgrad_side_branches
    tr.setup()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_state_dict(synthetic.passive_shapes(), 7).items()}
    tr.actor_critic.load_state_dict(sd)
    tr.actor_critic.train()
    tr.train_batch(*_batch(B, 11, dev))
    weights = {k: v.detach().cpu().clone() for k, v in tr.actor_critic.state_dict().items()}
    batch = _batch(B, 12, dev)
    tr.train_batch(*batch)
    torch.cuda.synchronize()
    assert tr._train_graph is not None and tr._train_graph.graph is not None, "the second batch did not run from the graph"
    opt = tr.optimizer
    grads, bad_alias, deferred = {}, [], 0
    index = {id(p): i for i, p in enumerate(opt._ps)}
    for name, p in tr.actor_critic.named_parameters():
        i = index[id(p)]
        off = opt._offsets[i]
        slot = opt.flat_g[off:off + p.numel()]
        grads[name] = slot.view(p.shape).cpu().clone()
        if p.dim() == 4:    # conv / transposed-conv weights: their gradients were deferred into their slots (functional._wgrad_launch)
            deferred += 1
            if p.grad is None or p.grad.data_ptr() != slot.data_ptr():
                bad_alias.append(name)
    assert deferred == 22
    return weights, [t.cpu() for t in batch], grads, bad_alias


def _oracle_grads(weights, batch):
    mix, gtb, gtm, tc = batch
    sd = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.double() if v.is_floating_point() else v)
          for k, v in weights.items()}
    bin_loss, mono_loss, _, _ = O.passive_losses(sd, mix.double(), tc, gtb.double(), gtm.double(), train_bn=True)
    (bin_loss + mono_loss).backward()
    return {k: v.grad for k, v in sd.items() if v.requires_grad}


@pytest.fixture(scope="module", params=[64, 5], ids=["B64", "B5"])
def step(request):
    weights, batch, grads, bad_alias = _graphed_step(request.param)
    return request.param, grads, _oracle_grads(weights, batch), bad_alias


def _rel_l2_and_scale(g, r):
    g, r = g.double().reshape(-1), r.double().reshape(-1)
    rr = float((r * r).sum())
    return float((g - r).norm()) / rr ** 0.5, float((g * r).sum()) / rr


def test_whole_step_gradients_match_fp64(step):
    B, grads, ref, _ = step
    assert set(grads) == set(ref)
    errs = {name: _rel_l2_and_scale(grads[name], ref[name]) for name in sorted(grads)}
    for name, (e, scale) in errs.items():
        print("B=%-3d %-55s relative L2 %.2e  scale-1 %+.2e" % (B, name, e, scale - 1.0))
    worst_l2, worst_scale = max(e for e, _ in errs.values()), max(abs(s - 1.0) for _, s in errs.values())
    print("passive step B=%d: worst per-tensor relative L2 %.2e, worst |scale - 1| %.2e over %d tensors" % (B, worst_l2, worst_scale, len(errs)))
    for name, (e, scale) in errs.items():
        assert e < L2_BOUND and abs(scale - 1.0) < SCALE_BOUND, (B, name, e, scale)
        # the bound rejects this tensor scaled by 0.99
        e99, s99 = _rel_l2_and_scale(ref[name] * 0.99, ref[name])
        assert not (e99 < L2_BOUND and abs(s99 - 1.0) < SCALE_BOUND)


def test_deferred_weight_gradients_alias_their_flat_slots(step):
    _, _, _, bad_alias = step
    assert not bad_alias, bad_alias
