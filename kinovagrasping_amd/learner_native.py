"""DDPGfD update without autograd (DDPGfD.train_batch, DDPGfD.py:219-367 of the reference), in three forms:

* **LDS-free MFMA kernels** (widths 256-256 / 128-128 / 64-64; `lds_free`): every forward, data-gradient and
  weight-gradient pass is a hand-written fp32-MFMA launch of libkinova_sim.so (csrc/ks_mlp.hip, mlp.py) that keeps its
  tiles in registers - one wave per 16 batch rows, <= 168 registers per lane, no LDS.  The simulator's stepping kernel
  holds all of every CU's LDS and 344 of the 512 registers per SIMD lane, so these waves are resident BESIDE it: the
  whole update runs in the stepping kernel's shadow on the matrix pipes and issue slots it leaves idle
  (pipeline.GraphedTrainer launches it on a second stream), instead of waiting for its workgroups to retire as the
  library GEMMs (which need LDS) must.  ~35 launches per update.
* **lean LDS-free MFMA kernels** (the reference's 400-300 and its partial tiles; `NativeDDPGfDUpdate(policy, lean=True)`, `lean_kernels`):
  the same passes on kr_mlp3_forward_lean / kr_mlp3_backward_lean + the generic kr_weight_grad_shadow.  The free-running rollout
  kernel at that width (k_rollout<25,19>) leaves 96 registers per SIMD lane, too few to keep a hidden layer in registers: these
  kernels write the first product's output (h1 / dz2) to global memory and stream it back with the weights, <= 96 registers, no
  scratch.  Opt-in: what pipeline.AsyncTrainer builds at 400-300; the default at that width stays the next form.
* **library GEMMs** (any width; the default at the reference's 400-300): explicit forward / backward GEMMs (PyTorch -> hipBLASLt)
  with the elementwise steps between them as single kernels (kr_relu_backward, ...), weight gradients written by the
  GEMMs straight into one flat gradient buffer per network; the forward-only target networks and the critic forward
  still go through the fused LDS kernel (kr_mlp3_forward) when the width has an instantiation.  ~75 launches.

Common to the three: one sequence of phases over the policy's critics - one for ddpgfd.DDPGfD, two for ddpgfd.TD3fD, whose target
actor's output is first smoothed in place (kr_target_smooth, in-kernel Philox noise keyed by the update count) - with ONE launch for the
targets and every critic's loss gradient (_loss_grad), one Adam launch per network (_adam) and one soft target update each
(kr_soft_update).  Which entry point a launch is follows from the policy alone, and each keeps the launch sequence and bits of the others
where they coincide:

* the loss gradient: kr_critic_grad for one critic, kr_twin_critic_grad (the bootstrap is the target critics' minimum) for two,
  kr_critic_grad_bounded for either when q_bounds or huber_delta is set on the policy (both None by default) - the bootstrapped value
  clamped to q_bounds, the TD loss Huber-shaped, the unset one of the two passed as its infinite value.  The priorities are handed the
  bootstrap the launch used: the target critic's own, or the [2R] minimum / clamped one it wrote;
* Adam: kr_adam_step; for TD3fD's delayed actor kr_adam_step_every (every policy_freq-th update); with max_grad_norm set (None by
  default) kr_grad_sqnorm (64 fp64 partial sums of the flat gradient buffer, no atomics) + kr_adam_step_clipped (clip_grad_norm_'s
  coefficient from them, then the step on g * coef; `every` is 1 but for TD3fD's actor), self.clip [3, 2] holding the (norm, coef) of
  actor, critic and critic2.  In the pipelined form the actor's norm is taken at the head, on the gradient buffer the body left.

* the behaviour-cloning term (the policy's bc_weight > 0; 0 by default: the launch sequence as it was): ONE launch, kr_bc_actor_grad, between
  the critic's data-gradient pass and the actor's own backward, adds the term's gradient on the demonstration rows (r >= demo_from) to
  dLoss/d(actor pre-activation) in place, from the actor's output and the Q the actor phase computes anyway; with q_filter one more critic
  forward, on the demonstration rows only (a contiguous tail), gives the filter's Q(s, a).  In the table form the rows are the B * H table
  rows, the actions tb.table_action, the first demonstration row b_agent * H.

* running observation normalisation (the policy's obs_norm; off by default: the launch sequence as it was): ONE kr_obs_stats_update in front
  of the update's prologue - the statistics take the windows' first states, gated on the device by the update count where freeze_after is set -,
  one kr_obs_normalize IN PLACE per gathered state buffer the update reads (the batch buffers are the samplers' copies of ring rows; the
  ring keeps raw observations, and so does nothing else: a caller that reuses a batch hands in a fresh copy), every pass as it was on those
  buffers, and ONE kr_fold_obs_norm behind the actor's Adam launch (phase_targets; pipelined: phase_head) that writes the first layer of the
  policy's acting copy (ddpgfd.DDPGfD.acting_flat: what the rollout acts with), the other layers copied - every update, so that the copy is
  fold(current actor, current statistics) under TD3fD's delayed actor and under a freeze too.

On a batch drawn as episode tables (replay.TableBatch; phase_critic_tables / phase_actor_tables, the LDS-free forms) the passes whose result
for a row depends on that row alone - the actor phase's forwards and data gradients, DDPGfD's target networks - run once per distinct state
(B * H table rows) instead of once per window that holds it (B * W * n rows), and the actor's weight gradients read their terms through an
index (kr_weight_grad_indexed): the window form's results bit for bit (docs/kernels.md).

All of these are LDS-free.  With world_size > 1 the flat gradient buffers are all-reduced directly (no pack /
unpack).  Same arithmetic as the reference (critic loss L1 + 0.5 LN on masked row means, actor loss -mean Q(s, pi(s))
over all n-step rows, Adam lr 1e-4 / default lr + weight_decay 1e-4, soft target update every 10th call);
tests/test_gpu_parity.py checks both forms against the autograd implementation (ddpgfd.DDPGfD.train_on_batch).  The
three `phase_*` methods mirror DDPGfD.phase_* so that pipeline.GraphedTrainer can capture them and run the gradient
exchange between them.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import mlp as _mlp
from . import sim as _sim


class _Net:
    """views of one MLP's flat parameter buffer + a flat gradient buffer of the same layout + Adam state; a trained network also has its
    optimizer's hyper-parameters and its row (`slot`) of NativeDDPGfDUpdate.clip / _partials"""

    def __init__(self, module, flat, optimizer=None, slot=None):
        if optimizer is not None:
            g = optimizer.param_groups[0]
            self.hyper = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
        self.slot = slot
        self.flat = flat
        self.grad = torch.zeros_like(flat)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.W, self.b, self.gW, self.gb = [], [], [], []
        off = 0
        for name in ("l1", "l2", "l3"):
            lin = getattr(module, name)
            for p, dst_p, dst_g in ((lin.weight, self.W, self.gW), (lin.bias, self.b, self.gb)):
                n = p.numel()
                assert p.data.data_ptr() == flat[off:off + n].data_ptr(), "parameters must be views of the flat buffer, in order"
                dst_p.append(p.data)
                dst_g.append(self.grad[off:off + n].view_as(p))
                off += n
        assert off == flat.numel()
        self.layers = list(zip(self.W, self.b))          # as mlp.py takes them


class NativeDDPGfDUpdate:
    def __init__(self, policy, lean=None):
        """lean: None keeps the form the width has by default (LDS-free kernels at 256-256 / 128-128 / 64-64, library GEMMs otherwise);
        True asks for an update without a single launch that needs LDS - the default LDS-free kernels where the width has them, the
        lean ones (mlp.LEAN_TILES: 400-300) where it does not, ValueError when it has neither."""
        assert policy.device.type == "cuda", "the learner glue kernels are GPU only"
        import os
        # a ddpgfd.TD3fD policy: a second critic pair, smoothed target actions, the actor's step on every policy_freq-th update
        self.td3 = "critic2" in policy._flat_params
        fork = os.environ.get("KS_LEARNER_FORK", "0") == "1"
        if self.td3 and fork:
            raise ValueError("NativeDDPGfDUpdate: the fork form (KS_LEARNER_FORK=1) has no TD3fD variant")
        # the bounded critic update (ddpgfd: q_bounds, huber_delta, max_grad_norm; None = the launch sequence as it was)
        q_bounds, huber_delta = getattr(policy, "q_bounds", None), getattr(policy, "huber_delta", None)
        self.max_grad_norm = getattr(policy, "max_grad_norm", None)
        self.bounded = q_bounds is not None or huber_delta is not None
        if (self.bounded or self.max_grad_norm is not None) and fork:
            raise ValueError("NativeDDPGfDUpdate: the fork form (KS_LEARNER_FORK=1) has no bounded variant (q_bounds / huber_delta / max_grad_norm)")
        inf = float("inf")
        self.q_lo, self.q_hi = (-inf, inf) if q_bounds is None else q_bounds
        self.huber_delta = inf if huber_delta is None else huber_delta
        # (norm, coef) of the last clipped step of actor, critic, critic2 (zeros while max_grad_norm is None) and kr_grad_sqnorm's partial sums
        self.clip = torch.zeros(3, 2, device=policy.device)
        self._partials = torch.zeros(3, _sim.KR_NORM_PARTS, dtype=torch.float64, device=policy.device) if self.max_grad_norm is not None else None
        # the behaviour-cloning term of the actor loss (ddpgfd: bc_weight, q_filter; 0 = the launch sequence as it was); with track_actor_loss
        # self.bc_loss holds the term and self.bc_pass the weighted share of demonstration states that passed the filter
        self.bc_weight, self.q_filter = float(getattr(policy, "bc_weight", 0.0)), bool(getattr(policy, "q_filter", False))
        self.bc_loss, self.bc_pass = torch.zeros((), device=policy.device), torch.zeros((), device=policy.device)
        # running observation normalisation (ddpgfd: obs_norm; None = the launch sequence as it was)
        self.obs_norm = getattr(policy, "obs_norm", None)
        if self.obs_norm is not None and fork:
            raise ValueError("NativeDDPGfDUpdate: the fork form (KS_LEARNER_FORK=1) has no obs_norm variant")
        self.p = policy
        self.lib = _sim.load_library()
        fp = policy._flat_params
        self.critic = _Net(policy.critic, fp["critic"], policy.critic_optimizer, slot=1)
        self.actor = _Net(policy.actor, fp["actor"], policy.actor_optimizer, slot=0)
        self.critic_t, self.actor_t = _Net(policy.critic_target, fp["critic_target"]), _Net(policy.actor_target, fp["actor_target"])
        self.critics, self.critic_targets = [self.critic], [self.critic_t]
        if self.td3:
            self.critic2 = _Net(policy.critic2, fp["critic2"], policy.critic2_optimizer, slot=2)
            self.critic2_t = _Net(policy.critic2_target, fp["critic2_target"])
            self.critics, self.critic_targets = [self.critic, self.critic2], [self.critic_t, self.critic2_t]
        # key of the target smoothing's in-kernel noise stream (counter: the update count); pipeline.GraphedTrainer hands over its sampler's
        self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self.it = torch.zeros(1, dtype=torch.long, device=policy.device)      # updates done (Adam step of both nets)
        # Pipelined form (phase_head): the actor's Adam step + soft target update of update k run at the START of update
        # k + 1.  `it_head` is k while that step is pending and 0 otherwise, so the head is a no-op when nothing is pending
        # (before the first update, or after finish_pending() has applied it eagerly, e.g. ahead of a checkpoint).
        self.it_head = torch.zeros(1, dtype=torch.long, device=policy.device)
        self.exchange = None             # exchange.PeerExchange when the ranks can map each other's memory (pipeline.GraphedTrainer)
        self.local_gradients = False     # pipeline.AsyncTrainer, replica_sync "average-per-launch": no per-update exchange, replicas averaged per launch
        self.pipelined = False        # set by pipeline.GraphedTrainer: the body marks its actor step pending for the next head
        policy._native = self                                                  # DDPGfD.save / load keep the Adam state in sync
        self.import_optimizer_state()
        self.losses = torch.zeros(6 if self.td3 else 3, device=policy.device)   # critic loss, L1, LN of the last update (TD3fD: then critic 2's)
        # How much of the update runs on the hand-written MFMA kernels of csrc/ks_mlp.hip (mlp.py):
        #  * fused_targets: the forward-only target networks (3200 rows) and the critic's forward (1600 rows, activations
        #    kept for the backward pass) as ONE launch each instead of three library GEMMs + glue;
        #  * shadow: ... in their LDS-free form, whose waves are resident beside the stepping kernel (which holds every
        #    CU's LDS) instead of waiting for its workgroups to retire;
        #  * lds_free: the backward passes too (mlp.mlp3_backward, mlp.weight_grad) - then no launch of the update needs
        #    LDS and the whole learner runs in the simulator's shadow.  Widths 256-256 / 128-128 / 64-64.
        # Otherwise (e.g. the reference's 400-300) the passes go through the library GEMMs (hipBLASLt).
        tl = [net.layers for net in (self.actor_t, self.critic_t)]
        ins = [net.W[0].shape[1] for net in (self.actor_t, self.critic_t)]
        mult = lambda k: all(w.shape[0] % k == 0 for w in self.critic.W[:2] + self.actor.W[:2])
        self.fused_targets = mult(4) and all(_mlp.supported(layers, d) for layers, d in zip(tl, ins))
        self.shadow = self.fused_targets and all(_mlp.supported(layers, d, shadow=True) for layers, d in zip(tl, ins))
        self.lds_free = self.shadow and mult(16) and os.environ.get("KS_EXP_LDSFREE", "1") == "1"
        # lean=True: no launch of the update may need LDS.  A width without the kernels above runs every pass - the 8000-row forwards
        # of the actor phase included - on the lean kernels (kr_mlp3_forward_lean / kr_mlp3_backward_lean: <= 96 registers per lane,
        # which is what k_rollout<25,19> leaves on a SIMD) and the generic kr_weight_grad_shadow.
        self.lean = bool(lean)
        self.lean_kernels = False
        if self.lean and not self.lds_free:
            nets = (self.actor, self.critic, self.actor_t, self.critic_t)
            if not all(_mlp.supported(net.layers, net.W[0].shape[1], lean=True) for net in nets):
                raise ValueError("NativeDDPGfDUpdate(lean=True): hidden widths %s have neither the LDS-free learner kernels (256-256 / 128-128 / "
                                 "64-64) nor the lean ones (400-300)" % (tuple(w.shape[0] for w in self.actor.W[:2]),))
            self.lean_kernels = self.fused_targets = self.lds_free = True
        self._form = dict(lean=True) if self.lean_kernels else dict(shadow=True)      # the LDS-free passes of mlp.py
        self._targets_form = self._form if self.lds_free else dict(shadow=self.shadow)
        # The 8000-row forwards of the actor phase stay on the library GEMMs unless the update is LDS-free: at that size
        # three large-tile GEMMs beat the 16-row-tile LDS kernel (measured 1.48 vs 1.44 ms per env-step in bench.py).
        self.fuse_critic_fwd, self.fuse_actor_fwd = True, False
        # diagnostics: the actor loss -mean_w Q(s, pi(s)) is not needed by the update (dLoss/dQ is constant); with
        # track_actor_loss it is evaluated from the Q of phase_actor's critic forward and kept in self.actor_loss
        self.track_actor_loss = False
        self.actor_loss = torch.zeros((), device=policy.device)
        # Fork / join inside a phase (round 5, LDS-free path): the launches of an update that do not depend on each other - the target
        # networks' pass beside the critic's forward, the three weight-gradient launches of a network beside its data-gradient pass -
        # go to two side streams that leave from and rejoin the phase's stream (under stream capture: parallel branches of the graph).
        # Every launch of the LDS-free update is one latency-bound wave per 16 rows (87 us whatever the batch, ks_mlp.hip) on a few
        # hundred of the 1024 SIMDs: branches run at the same time instead of one after the other.
        # OFF by default (KS_LEARNER_FORK=1 turns it on).  Measured, round 5, one MI355X: the update replayed ALONE 0.878 -> 0.733 ms
        # (10.4 GFLOP: 7.5 % -> 9.0 % of the fp32 MFMA peak), bit-identical results (tests/test_gpu_learner_state.py) - but beside the
        # persistent rollout kernel the training step went from 1.34 to 2.09 ms per env-step (3.05 -> 1.96 M env-steps/s) and episodes were
        # dropped: three learner launches at a time compete with the rollout's waves for the SIMDs' issue slots, and the update is off
        # the critical path at one update per env-step anyway.  Kept for learner-bound regimes (updates_per_step >= 2 in lock step).
        self.fork = self.lds_free and fork
        self._sides = [torch.cuda.Stream(policy.device) for _ in range(2)] if self.fork else []

    # -- helpers ------------------------------------------------------------------------------------------------------
    def _branch(self, k):
        """context, the fork form: side stream k, ordered behind everything enqueued on the current stream so far (a fork); _join() brings
        it back.  Otherwise: the current stream."""
        if not self.fork:
            return contextlib.nullcontext()
        cur = torch.cuda.current_stream(self.p.device)
        side = self._sides[k]
        side.wait_stream(cur)
        return torch.cuda.stream(side)

    def _join(self, *ks):
        if self.fork:
            cur = torch.cuda.current_stream(self.p.device)
            for k in ks:
                cur.wait_stream(self._sides[k])

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.p.device).cuda_stream)

    @staticmethod
    def _chk(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")

    @staticmethod
    def _lin_relu(net, k, x):
        return torch._addmm_activation(net.b[k], x, net.W[k].t())

    def _actor_forward(self, net, x):
        h1 = self._lin_relu(net, 0, x)
        h2 = self._lin_relu(net, 1, h1)
        a = torch.addmm(net.b[2], h2, net.W[2].t()).sigmoid_().mul_(self.p.max_action)
        return h1, h2, a

    def _relu_bwd(self, act, grad):
        self._chk(self.lib.kr_relu_backward(grad.numel(), _sim._ptr(act), _sim._ptr(grad), self._st()), "kr_relu_backward")

    def _adam(self, net, step, every=None):
        """net's Adam step for the update counted by `step`; every (TD3fD's actor): on every `every`-th update only, numbered step / every.
        With max_grad_norm behind the global gradient-norm clip: the squared norm as 64 fp64 partial sums, then the step on g * coef."""
        P, n = _sim._ptr, net.flat.numel()
        state = (n, P(net.flat), P(net.grad), P(net.exp_avg), P(net.exp_avg_sq), P(step))
        if self.max_grad_norm is not None:
            parts = self._partials[net.slot]
            self._chk(self.lib.kr_grad_sqnorm(n, P(net.grad), P(parts), self._st()), "kr_grad_sqnorm")
            self._chk(self.lib.kr_adam_step_clipped(*state, 1 if every is None else every, P(parts), self.max_grad_norm, *net.hyper,
                                                    P(self.clip[net.slot]), self._st()), "kr_adam_step_clipped")
        elif every is not None:
            self._chk(self.lib.kr_adam_step_every(*state, every, *net.hyper, self._st()), "kr_adam_step_every")
        else:
            self._chk(self.lib.kr_adam_step(*state, *net.hyper, self._st()), "kr_adam_step")

    def _adam_actor(self, step):
        self._adam(self.actor, step, every=self.p.policy_freq if self.td3 else None)

    def _obs_stats(self, x, lda, weight):
        """obs_norm, in front of the prologue (self.it: the updates done): the statistics take the rows of x [R, >= S] whose weight is not 0"""
        on, P = self.obs_norm, _sim._ptr
        assert x.dtype == torch.float32 and x.stride(-1) == 1 and (weight is None or (weight.dtype == torch.float32 and weight.is_contiguous()))
        self._chk(self.lib.kr_obs_stats_update(x.shape[0], on.dim, P(x), lda, P(weight), P(self.it), on.freeze_after or 0, P(on.count), P(on.mean), P(on.m2),
                                               P(on.mean32), P(on.inv32), on.eps, self._st()), "kr_obs_stats_update")

    def _obs_normalize(self, *buffers):
        """obs_norm: each gathered state buffer [..., S] (contiguous) -> (x - mean32) * inv32, in place"""
        on, P = self.obs_norm, _sim._ptr
        for x in buffers:
            assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == on.dim
            self._chk(self.lib.kr_obs_normalize(x.numel() // on.dim, on.dim, P(x), on.dim, P(on.mean32), P(on.inv32), self._st()), "kr_obs_normalize")

    def _fold(self):
        """obs_norm, behind the actor's Adam launch: the policy's acting copy <- the actor with the normalisation folded into its first layer"""
        if self.obs_norm is None:
            return
        on, P, a = self.obs_norm, _sim._ptr, self.actor
        acting = self.p.acting_flat()
        (w1, b1), _, _ = self.p.acting_layers()
        h1, in_dim = a.W[0].shape
        self._chk(self.lib.kr_fold_obs_norm(h1, in_dim, on.dim, P(a.W[0]), P(a.b[0]), P(on.mean32), P(on.inv32), P(w1), P(b1), self._st()), "kr_fold_obs_norm")
        first = h1 * in_dim + h1
        acting[first:].copy_(a.flat[first:])

    def _soft_updates(self, it):
        pol, P = self.p, _sim._ptr
        for net, tgt in zip(self.critics + [self.actor], self.critic_targets + [self.actor_t]):
            self._chk(self.lib.kr_soft_update(net.flat.numel(), P(net.flat), P(tgt.flat), pol.tau, P(it), pol.network_repl_freq, self._st()),
                      "kr_soft_update")

    # -- optimizer state <-> torch.optim.Adam (the reference's 4-file checkpoint keeps it: DDPGfD.py:371-382) ------------
    def _optim_pairs(self):
        pairs = ((self.actor, self.p.actor_optimizer), (self.critic, self.p.critic_optimizer))
        return pairs + (((self.critic2, self.p.critic2_optimizer),) if self.td3 else ())

    def export_optimizer_state(self):
        """Make policy.{actor,critic}_optimizer.state describe the native Adam state: exp_avg / exp_avg_sq are VIEWS of the
        flat moment buffers (they stay current), `step` is the number of updates applied (TD3fD's delayed actor: the number of steps it
        took, it // policy_freq).  Applies a pending pipelined actor step first, so that both networks are at the same update."""
        torch.cuda.synchronize(self.p.device)          # a pipelined update may still be running on the learner's stream
        self.finish_pending()
        it = int(self.it.item())
        for net, opt in self._optim_pairs():
            step = float(it // self.p.policy_freq if (self.td3 and net is self.actor) else it)
            off = 0
            for p in opt.param_groups[0]["params"]:
                n = p.numel()
                cap = opt.param_groups[0].get("capturable", False)
                opt.state[p] = {"step": torch.tensor(step, dtype=torch.float32, device=p.device if cap else "cpu"),
                                "exp_avg": net.exp_avg[off:off + n].view_as(p), "exp_avg_sq": net.exp_avg_sq[off:off + n].view_as(p)}
                off += n

    def import_optimizer_state(self):
        """Adopt the state the torch optimizers hold (after DDPGfD.load, or after autograd updates): moments into the flat
        buffers, the update counter from `step`.  No state = a fresh optimizer (zeros)."""
        steps = []
        for net, opt in self._optim_pairs():
            off = 0
            for p in opt.param_groups[0]["params"]:
                n = p.numel()
                stt = opt.state.get(p, None)
                if stt:
                    if stt["exp_avg"].data_ptr() != net.exp_avg[off:off + n].data_ptr():
                        net.exp_avg[off:off + n].copy_(stt["exp_avg"].reshape(-1))
                        net.exp_avg_sq[off:off + n].copy_(stt["exp_avg_sq"].reshape(-1))
                    steps.append((int(float(stt["step"])), net is self.actor))
                off += n
        if steps and self.td3:
            # the critics count the updates; the delayed actor has taken every policy_freq-th of them
            critics = [s for s, is_actor in steps if not is_actor]
            its = critics if critics else [s * self.p.policy_freq for s, _ in steps]
            assert min(its) == max(its) and all(s == its[0] // self.p.policy_freq for s, is_actor in steps if is_actor), \
                "actor and critic optimizers are at different steps"
            steps = its
        elif steps:
            steps = [s for s, _ in steps]
            assert min(steps) == max(steps), "actor and critic optimizers are at different steps"
        if steps:
            self.it.fill_(steps[0])
            self.it_head.zero_()
            self.p.total_it = steps[0]

    @torch.no_grad()
    def finish_pending(self):
        """apply the pipelined actor step that is still waiting for the next update's head (no-op otherwise)"""
        self.phase_head()
        self.it_head.zero_()

    def _weight_grads(self, net, x, h1, h2, dz3):
        """dz3: gradient at the last layer's pre-activation; fills net.grad, returns nothing"""
        torch.mm(dz3.t(), h2, out=net.gW[2])
        torch.sum(dz3, 0, out=net.gb[2])
        dh2 = torch.mm(dz3, net.W[2])
        self._relu_bwd(h2, dh2)
        torch.mm(dh2.t(), h1, out=net.gW[1])
        torch.sum(dh2, 0, out=net.gb[1])
        dh1 = torch.mm(dh2, net.W[1])
        self._relu_bwd(h1, dh1)
        torch.mm(dh1.t(), x, out=net.gW[0])
        torch.sum(dh1, 0, out=net.gb[0])

    # -- the three phases ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def phase_critic(self, state, action, next_state, reward, weight=None, next_ends=None, priorities=None, target_noise=None):
        """obs_norm: the statistics take state[:, 0] and `state` and `next_state` (`next_ends` when given: next_state is then not read) are
        normalised IN PLACE - phase_actor takes the same `state` buffer as it is then.
        The target actor's forward (TD3fD: kr_target_smooth on its output), every target critic on that action, every critic's forward,
        ONE loss-gradient launch (_loss_grad), the backward and weight-gradient passes per critic -> the critics' .grad.  Returns (critic
        loss, L1, LN) per critic, views of self.losses.  priorities (prioritized replay): a callable (q, tq1, reward, weight) issued right
        after the loss-gradient launch on that kernel's own operands - the first critic's Q and the bootstrap the launch used -
        DeviceEpisodeReplay.update_priorities with the batch's `picked` bound; None: the launch sequence has no such step.
        target_noise [2R, 4]: the smoothing's N(0, 1) draws; None: the in-kernel stream keyed by (self.seed, self.it)."""
        pol, P = self.p, _sim._ptr
        R = reward.shape[0]
        if weight is None:
            weight = torch.ones(R, device=reward.device)
        if self.obs_norm is not None:
            assert state.is_contiguous()
            self._obs_stats(state[:, 0], state.shape[1] * state.shape[2], weight)
            self._obs_normalize(state, next_state if next_ends is None else next_ends)
        # one launch: update counter, sum of the row weights, dLoss/dQ of the actor loss (and, pipelined, the pending mark)
        self.weight, self.wsum = weight, torch.empty(1, device=reward.device)
        self.dq_actor = torch.empty(R * pol.n, 1, device=reward.device)
        self._chk(self.lib.kr_update_prologue(R, pol.n, P(weight), P(self.wsum), P(self.dq_actor), P(self.it), P(self.it_head),
                                              int(self.pipelined), self._st()), "kr_update_prologue")
        # both target evaluations (1-step: next_state[:, 0], n-step: next_state[:, -1]) in one pass of the target nets
        # (next_ends: the sampler's own [2R, S] block of exactly these rows, kr_sample_windows_draw)
        nx = torch.cat([next_state[:, 0], next_state[:, -1]], 0) if next_ends is None else next_ends
        return self._critic_phase(state[:, 0], action[:, 0], reward, weight, lambda: self._window_targets(nx, target_noise), priorities)

    def _window_targets(self, nx, target_noise):
        """every target critic's Q on the [2R] rows nx (the windows' first next states, then their last)"""
        ta = self._target_actions(nx, target_noise)
        return [self._target_q(ct, nx, ta) for ct in self.critic_targets]

    def _table_targets(self, tb):
        """DDPGfD on episode tables: the target networks on the T table rows of table_next - every next state once - and the [2R] rows the
        loss gradient takes gathered from their Q (kr_gather_table_q).  Row-independent kernels: the bits of _window_targets."""
        P, R = _sim._ptr, tb.weight.shape[0]
        tq_table = self._window_targets(tb.table_next, None)[0]
        tq = tq_table.new_empty(2 * R, 1)
        self._chk(self.lib.kr_gather_table_q(R, tb.n_steps, P(tb.row_table), P(tq_table), P(tq), self._st()), "kr_gather_table_q")
        return [tq]

    @torch.no_grad()
    def phase_critic_tables(self, tb, priorities=None, target_noise=None):
        """phase_critic on a replay.TableBatch (LDS-free forms only): the same launches at R rows for the critics; the target networks see
        the T = B * H table rows instead of 2R window ends (DDPGfD; TD3fD's smoothing noise is keyed by the row of [2R]: it keeps those
        rows, tb.next_ends).  The prologue writes dLoss/dQ of the actor loss per table row and the window states' table rows for
        phase_actor_tables.  Every result is bit for bit phase_critic's on tb.windows()."""
        assert self.lds_free, "the table form runs on the LDS-free kernels"
        pol, P = self.p, _sim._ptr
        R, T = tb.weight.shape[0], tb.table_state.shape[0]
        assert tb.n_steps == pol.n and (not self.td3 or tb.next_ends is not None)
        if self.obs_norm is not None:
            self._obs_stats(tb.state0, tb.state0.shape[1], tb.weight)
            self._obs_normalize(tb.table_state, tb.state0, tb.next_ends if self.td3 else tb.table_next)     # (TD3fD does not read table_next)
        self.weight, self.wsum = tb.weight, torch.empty(1, device=tb.weight.device)
        self.dq_table = torch.empty(T, 1, device=tb.weight.device)
        self.row_index = torch.empty(R * pol.n, dtype=torch.int32, device=tb.weight.device)
        self._chk(self.lib.kr_update_prologue_tables(R, pol.n, T // tb.horizon, tb.horizon, P(tb.weight), P(tb.slot_weight), P(tb.row_table), P(self.wsum),
                                                     P(self.dq_table), P(self.row_index), P(self.it), P(self.it_head), int(self.pipelined), self._st()),
                  "kr_update_prologue_tables")
        targets = (lambda: self._window_targets(tb.next_ends, target_noise)) if self.td3 else (lambda: self._table_targets(tb))
        return self._critic_phase(tb.state0, tb.action0, tb.reward, tb.weight, targets, priorities)

    def _critic_phase(self, s0, a0, reward, weight, targets, priorities):
        """phase_critic behind its prologue: s0 / a0 [R, *] the windows' first state and action, targets() the target critics' [2R] Q"""
        with self._branch(0):       # (the fork form: the target networks, 3200 rows each, beside the critic's own forward on the phase's stream)
            tqs = targets()
        qs, saved = zip(*[self._critic_forward(c, s0, a0) for c in self.critics])
        self._join(0)
        reward = reward.contiguous()
        dqs, boot = self._loss_grad(qs, tqs, reward, weight)
        if priorities is not None:
            priorities(qs[0], boot, reward, weight)         # the bootstrap the update used
        for c, dq, sv in zip(self.critics, dqs, saved):
            self._critic_backward(c, dq, sv)
        return tuple(self.losses[k] for k in range(3 * len(self.critics)))

    # the passes of phase_critic, per network (TD3fD runs the critic's twice)
    def _target_actions(self, nx, target_noise):
        pol, P = self.p, _sim._ptr
        if self.fused_targets:
            # forward-only networks: one fused fp32-MFMA launch each (mlp.mlp3_forward) instead of 3 GEMMs + glue
            ta = _mlp.mlp3_forward(self.actor_t.layers, nx, act=_mlp.ACT_SIGMOID, scale=pol.max_action, **self._targets_form)
        else:
            ta = self._actor_forward(self.actor_t, nx)[2]
        if self.td3:
            assert ta.is_contiguous() and (target_noise is None or (target_noise.is_contiguous() and target_noise.dtype == torch.float32 and
                                                                    target_noise.device == ta.device and tuple(target_noise.shape) == tuple(ta.shape)))
            self._chk(self.lib.kr_target_smooth(ta.shape[0], P(ta), P(target_noise), self.seed, None if target_noise is not None else P(self.it),
                                                pol.policy_noise, pol.noise_clip, pol.max_action, self._st()), "kr_target_smooth")
        return ta

    def _target_q(self, ct, nx, ta):
        if self.fused_targets:
            return _mlp.mlp3_forward(ct.layers, nx, ta, act=_mlp.ACT_NONE, **self._targets_form)
        return torch.addmm(ct.b[2], self._lin_relu(ct, 1, self._lin_relu(ct, 0, torch.cat([nx, ta], 1))), ct.W[2].t())

    def _loss_grad(self, qs, tqs, reward, weight):
        """ONE launch: the targets and every critic's dLoss/dQ from the critics' Q and their target critics' [2R] (1-step rows, then n-step),
        the losses -> self.losses.  kr_critic_grad for one critic, kr_twin_critic_grad for two, kr_critic_grad_bounded for either when
        self.bounded.  Returns the dqs and the bootstrap the launch used, which `priorities` must see: the target critic's own, or the [2R]
        the kernel wrote where it took the minimum or clamped."""
        pol, P, R = self.p, _sim._ptr, reward.shape[0]
        twin = len(qs) == 2
        dqs = [torch.empty_like(q) for q in qs]
        boot = qs[0].new_empty(2 * R) if twin or self.bounded else tqs[0]
        pair = lambda xs: [P(x) for x in xs] + [None] * (2 - len(xs))
        nets = pair(qs) + pair(tqs) + pair([tq[R:] for tq in tqs])                # q1, q2, tq1_a, tq1_b, tqn_a, tqn_b
        batch = (P(reward), P(weight), P(self.wsum), pol.discount)
        if self.bounded:
            name, args = "kr_critic_grad_bounded", (*nets, *batch, self.q_lo, self.q_hi, self.huber_delta, *pair(dqs), P(boot))
        elif twin:
            name, args = "kr_twin_critic_grad", (*nets, *batch, *pair(dqs), P(boot))
        else:
            name, args = "kr_critic_grad", (nets[0], nets[2], nets[4], *batch, P(dqs[0]))
        self._chk(getattr(self.lib, name)(R, pol.n, *args, P(self.losses), self._st()), name)
        return dqs, boot

    def _critic_forward(self, c, s0, a0):
        """Q of the windows' first rows s0 / a0; returns (q, what _critic_backward needs)"""
        R = s0.shape[0]
        if self.lds_free:
            # the whole critic step without LDS: forward, loss gradient, data and weight gradients (csrc/ks_mlp.hip)
            h1, h2 = s0.new_empty(R, c.W[0].shape[0]), s0.new_empty(R, c.W[1].shape[0])
            q = _mlp.mlp3_forward(c.layers, s0, a0, act=_mlp.ACT_NONE, h1_out=h1, h2_out=h2, **self._form)
            return q, (s0, a0, h1, h2)
        x0 = torch.cat([s0, a0], 1)
        if self.fused_targets and self.fuse_critic_fwd:
            h1, h2 = x0.new_empty(R, c.W[0].shape[0]), x0.new_empty(R, c.W[1].shape[0])
            q = _mlp.mlp3_forward(c.layers, s0, a0, act=_mlp.ACT_NONE, h1_out=h1, h2_out=h2, **self._targets_form)
        else:
            h1 = self._lin_relu(c, 0, x0)
            h2 = self._lin_relu(c, 1, h1)
            q = torch.addmm(c.b[2], h2, c.W[2].t())
        return q, (x0, h1, h2)

    def _critic_backward(self, c, dq, saved):
        """dq = dLoss/dQ -> c.grad"""
        if self.lds_free:
            self._backward(c, dq, *saved)
        else:
            self._weight_grads(c, *saved, dq)

    def _backward(self, net, dz3, x, xa, h1, h2, idx=None):
        """LDS-free: dz3 = the gradient at the pre-activation of net's last layer, [x, xa] its input -> net.grad.  The fork form: the last
        layer's weight gradient needs dz3 only and the second's dz2 only: on the side streams, beside the data-gradient pass and the first's.
        idx (the table form): the weight gradients' terms are the rows idx[r] of these tensors (mlp.weight_grad)."""
        last = lambda: _mlp.weight_grad(dz3, h2, None, net.gW[2], net.gb[2], idx=idx)
        if self.fork:
            with self._branch(0):
                last()
        dz2, dz1, _ = _mlp.mlp3_backward(net.layers, dz3, h1, h2, lean=self.lean_kernels)
        if not self.fork:
            last()
        with self._branch(1):
            _mlp.weight_grad(dz2, h1, None, net.gW[1], net.gb[1], idx=idx)
        _mlp.weight_grad(dz1, x, xa, net.gW[0], net.gb[0], idx=idx)
        self._join(0, 1)

    def _bc_rows(self, action, demo_from, window_rows, per):
        """None while bc_weight is 0; else (demo [rows, 4], the first demonstration row among the actor phase's rows, demo_from) - per =
        (window rows, actor-phase rows) of one unit of the batch: (1, n) for window states, (W, H) for a batch slot's table rows"""
        if not self.bc_weight > 0:
            return None
        if action is None or demo_from is None:
            raise ValueError("bc_weight > 0: the actor phase needs the batch's actions and demo_from, the first demonstration row")
        d = int(demo_from)
        if not 0 <= d <= window_rows:
            raise ValueError("demo_from must lie in [0, rows]")
        assert d % per[0] == 0, "the table form: demo_from is a whole number of batch slots (b_agent * W window rows)"
        demo = action.reshape(-1, action.shape[-1])
        assert demo.dtype == torch.float32 and demo.is_contiguous() and demo.shape[1] == 4
        return demo, d // per[0] * per[1], d

    def _critic_q(self, s, a, out):
        """critic 1's Q on the rows (s, a) -> out [rows, 1], on the kernels of the form in use (the filter's Q(s, a) on the demonstration rows)"""
        c = self.critic
        if self.lds_free:
            _mlp.mlp3_forward(c.layers, s, a, act=_mlp.ACT_NONE, out=out, **self._form)
        elif self.fused_targets and self.fuse_actor_fwd:
            _mlp.mlp3_forward(c.layers, s, a, act=_mlp.ACT_NONE, out=out)
        else:
            torch.addmm(c.b[2], self._lin_relu(c, 1, self._lin_relu(c, 0, torch.cat([s, a], 1))), c.W[2].t(), out=out)

    def _bc(self, sa, pi, q_pi, dq, dz3, n, idx, demo, first, demo_from):
        """the behaviour-cloning term on the actor phase's rows (_bc_rows): dz3 += its gradient on the rows r >= first (kr_bc_actor_grad, one
        launch; with q_filter behind the critic's forward on those rows' demonstrated actions).  demo_from, in window rows, is what the
        tracked pass share is normalised by."""
        P, rows = _sim._ptr, sa.shape[0]
        assert demo.shape[0] == rows and 0 <= first <= rows and pi.is_contiguous() and dz3.is_contiguous() and tuple(dz3.shape) == (rows, 4)
        q_demo = None
        if self.q_filter:
            q_demo = pi.new_empty(rows, 1)                   # (the kernel reads the rows r >= first only)
            if first < rows:
                self._critic_q(sa[first:], demo[first:], q_demo[first:])
        sq, passed = pi.new_empty(rows), pi.new_empty(rows)
        self._chk(self.lib.kr_bc_actor_grad(rows, first, P(pi), P(demo), P(q_demo), P(q_pi) if self.q_filter else None, P(dq), self.bc_weight,
                                            self.p.max_action, P(dz3), P(sq), P(passed), self._st()), "kr_bc_actor_grad")
        if self.track_actor_loss:
            if idx is not None:
                rows_of = idx.long().clamp(min=0)
                sq, passed = sq[rows_of], passed[rows_of]
            self._set_bc_loss(sq, passed, n, demo_from)

    def _set_bc_loss(self, sq, passed, n, demo_from):
        """bc_weight sum_{r >= demo_from} w_r sum_k f_rk |pi - a|^2 / (sum(w) n), added to the tracked actor loss, and the weighted share of
        demonstration states with f = 1; sq and passed per window state (zero on the agent rows)"""
        w = self.weight
        self.bc_loss = self.bc_weight * (sq.view(-1, n).sum(1) * w).sum() / (self.wsum[0] * float(n))
        self.bc_pass = (passed.view(-1, n).sum(1) * w).sum() / (w[demo_from:].sum() * float(n)).clamp_min(torch.finfo(torch.float32).tiny)
        self.actor_loss = self.actor_loss + self.bc_loss

    @torch.no_grad()
    def phase_actor(self, state, weight=None, action=None, demo_from=None):
        """critic Adam step, then the actor loss -mean_w Q(s, pi(s)) over all n-step rows -> self.actor.grad; with the policy's bc_weight > 0
        plus the behaviour-cloning term on the rows r >= demo_from of `action` [R, n, 4] (ValueError without them, before any launch)"""
        pol, P = self.p, _sim._ptr
        n = state.shape[1]
        bc = self._bc_rows(action, demo_from, state.shape[0], (1, n))
        for net in self.critics:
            self._adam(net, self.it)
        sa = state.reshape(-1, state.shape[2])
        a_, c = self.actor, self.critic
        if self.lds_free:
            self._actor_rows(sa, self.dq_actor, n, None, bc)
            return None
        if self.fused_targets and self.fuse_actor_fwd:
            rows = sa.shape[0]
            ha1, ha2 = sa.new_empty(rows, a_.W[0].shape[0]), sa.new_empty(rows, a_.W[1].shape[0])
            a = _mlp.mlp3_forward(a_.layers, sa, act=_mlp.ACT_SIGMOID, scale=pol.max_action, h1_out=ha1, h2_out=ha2)
            hc1, hc2 = sa.new_empty(rows, c.W[0].shape[0]), sa.new_empty(rows, c.W[1].shape[0])
            _mlp.mlp3_forward(c.layers, sa, a, act=_mlp.ACT_NONE, h1_out=hc1, h2_out=hc2)      # Q itself is not needed: dLoss/dQ is constant
        else:
            ha1, ha2, a = self._actor_forward(a_, sa)
            hc1 = self._lin_relu(c, 0, torch.cat([sa, a], 1))
            hc2 = self._lin_relu(c, 1, hc1)
        q = torch.addmm(c.b[2], hc2, c.W[2].t()) if (self.track_actor_loss or (bc is not None and self.q_filter)) else None
        if self.track_actor_loss:
            self._set_actor_loss(q, n)
        # d(-sum_r w_r sum_k Q_rk / (sum(w) n)) / dQ_rk  (kr_update_prologue)
        dq = self.dq_actor
        dh2 = torch.mm(dq, c.W[2])
        self._relu_bwd(hc2, dh2)
        dh1 = torch.mm(dh2, c.W[1])
        self._relu_bwd(hc1, dh1)
        da = torch.mm(dh1, c.W[0][:, sa.shape[1]:])                       # only the action columns of the critic's first layer
        self._chk(self.lib.kr_sigmoid_scale_backward(da.numel(), P(a), pol.max_action, P(da), self._st()), "kr_sigmoid_scale_backward")
        if bc is not None:
            self._bc(sa, a, q, dq, da, n, None, *bc)
        self._weight_grads(a_, sa, ha1, ha2, da)
        return None

    def _actor_rows(self, sa, dq, n, idx, bc=None):
        """LDS-free: the actor phase's passes on the states sa with dLoss/dQ dq per row -> self.actor.grad.  idx None: sa are the window
        states themselves; else (the table form) sa are table rows, each evaluated once, and the sums over the window states - the weight
        gradients, the tracked loss - read row idx[r] for state r (-1: a padding row's, which adds exact zeros in the window form).
        bc (_bc_rows): the behaviour-cloning term's gradient joins dz3 before the actor's own backward."""
        pol, a_, c = self.p, self.actor, self.critic
        rows = sa.shape[0]
        al, cl = a_.layers, c.layers
        ha1, ha2 = sa.new_empty(rows, a_.W[0].shape[0]), sa.new_empty(rows, a_.W[1].shape[0])
        a = _mlp.mlp3_forward(al, sa, act=_mlp.ACT_SIGMOID, scale=pol.max_action, h1_out=ha1, h2_out=ha2, **self._form)
        hc1, hc2 = sa.new_empty(rows, c.W[0].shape[0]), sa.new_empty(rows, c.W[1].shape[0])
        q = _mlp.mlp3_forward(cl, sa, a, act=_mlp.ACT_NONE, h1_out=hc1, h2_out=hc2, **self._form)       # Q itself is not needed
        if self.track_actor_loss:
            self._set_actor_loss(q if idx is None else q[idx.long().clamp(min=0)], n)
        # dLoss/d(actor pre-activation): through the critic to its action inputs, then through 0.8 * sigmoid
        _, _, dz3 = _mlp.mlp3_backward(cl, dq, hc1, hc2, want_dz=False, dx_cols=(sa.shape[1], a.shape[1]), act_out=a, scale=pol.max_action, lean=self.lean_kernels)
        if bc is not None:
            self._bc(sa, a, q, dq, dz3, n, idx, *bc)
        self._backward(a_, dz3, sa, None, ha1, ha2, idx=idx)

    @torch.no_grad()
    def phase_actor_tables(self, tb, demo_from=None):
        """phase_actor on a replay.TableBatch, after phase_critic_tables: the four per-row passes (actor and critic forward, the critic's data
        gradient to the action columns, the actor's data gradient) run on the T = B * H table rows - a row's result depends on that row's
        inputs only, and every real window of batch slot b carries the same dq -, the actor's three weight gradients keep their R * n
        terms, order and chunks and read each term through its table row.  self.actor.grad is bit for bit phase_actor's on tb.windows()
        (padding rows, which add exact zeros there, read as zeros here).  demo_from (the policy's bc_weight > 0): the first demonstration
        WINDOW row, b_agent * W, as phase_actor takes it; the term's rows here are the table rows from b_agent * H on, its actions
        tb.table_action and its coefficient dq_table - the indexed weight gradients give each table row its multiplicity."""
        assert self.lds_free, "the table form runs on the LDS-free kernels"
        bc = self._bc_rows(tb.table_action, demo_from, tb.weight.shape[0], (tb.horizon - tb.n_steps, tb.horizon))
        for net in self.critics:
            self._adam(net, self.it)
        self._actor_rows(tb.table_state, self.dq_table, tb.n_steps, self.row_index, bc)

    def _set_actor_loss(self, q, n):
        """-sum_r w_r sum_k Q_rk / (sum(w) n)  (DDPGfD.py:341: -critic(state, actor(state)).mean())"""
        self.actor_loss = -(q.view(-1, n).sum(1) * self.weight).sum() / (self.wsum[0] * float(n))

    @torch.no_grad()
    def phase_head(self):
        """Pipelined form of phase_targets: applied at the START of the next update (pipeline.GraphedTrainer), so that
        the actor's weights change at one known, early point of every update instead of at its end.  Gated on the device
        counter `it_head` (set by mark_pending at the end of an update's body, cleared here): a no-op when no actor step is
        pending."""
        self._adam_actor(self.it_head)
        self._fold()
        self._soft_updates(self.it_head)
        # (no clearing here: in the pipelined form every body re-marks it_head and a head always runs between two bodies;
        # finish_pending, the eager caller, clears it)

    @torch.no_grad()
    def phase_targets(self):
        """actor Adam step + soft target update on every network_repl_freq-th update"""
        self._adam_actor(self.it)
        self._fold()
        self.p.total_it += 1
        self._soft_updates(self.it)

    def allreduce(self, net):
        """average the flat gradient buffer of `net` ("critic" / "actor") over the process group (RCCL), in place"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(self.p.process_group)
        if world == 1 or self.local_gradients:
            return
        g = getattr(self, net).grad
        if self.exchange is not None:
            self.exchange.allreduce_mean(g)        # LDS-free, over peer-mapped memory: runs beside the stepping kernel (exchange.py)
            return
        dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.p.process_group)
        g.div_(world)

    def train_on_tables(self, tb, target_noise=None, demo_from=None):
        """train_on_batch on a replay.TableBatch: bit for bit train_on_batch(*tb.windows()) (the sign of an exactly-zero Adam moment aside)"""
        losses = self.phase_critic_tables(tb, target_noise=target_noise)
        self.allreduce("critic")
        if self.td3:
            self.allreduce("critic2")
        self.phase_actor_tables(tb, demo_from)
        self.allreduce("actor")
        self.phase_targets()
        return losses

    def train_on_batch(self, state, action, next_state, reward, weight=None, target_noise=None, demo_from=None):
        losses = self.phase_critic(state, action, next_state, reward, weight, target_noise=target_noise)
        self.allreduce("critic")
        if self.td3:
            self.allreduce("critic2")
        self.phase_actor(state, weight, action, demo_from)
        self.allreduce("actor")
        self.phase_targets()
        return losses
