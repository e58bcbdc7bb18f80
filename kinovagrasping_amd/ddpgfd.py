"""DDPG-from-Demonstration learner (L1-L3) for the batched simulator.

Mirrors gym-kinova-gripper/DDPGfD.py of the reference: Actor `max_action*sigmoid(l3 relu(l2 relu(l1 s)))`
(DDPGfD.py:15-32), Critic on [state, action] (DDPGfD.py:35-50), `select_action` (71-73) and the working
update `train_batch` (219-367): 1-step + n-step critic targets, lambda_1 = 0.5, Adam (actor lr 1e-4,
critic default lr + weight_decay 1e-4, DDPGfD.py:57,61), soft target update every 10th call
(360-366).  The broken full-episode `train` (SURVEY note N2) is not reproduced.

Layer names (l1, l2, l3) and shapes match the reference so its 4-file checkpoints
(`<prefix>_{actor,critic,actor_optimizer,critic_optimizer}`, DDPGfD.py:371-382) load unchanged.  Hidden
widths are parameters: 400-300 is the reference (parity), 256-256 is what BASELINE.json benchmarks.

MI355X notes: everything stays on the GPU (no per-step host round trip as in DDPGfD.py:71-73); the
GEMMs run on the matrix cores through PyTorch-ROCm (hipBLASLt); with world_size > 1 the gradients of
both networks are averaged with ONE all-reduce over a flat fp32 buffer (RCCL over xGMI).

`TD3fD(DDPGfD)` is the same learner with TD3's remedy for the single critic's over-estimation (twin critics with the minimum in the
target, noise-smoothed target actions, a delayed actor); `DDPGfD` itself is unchanged by it, and a TD3fD checkpoint loads into a
DDPGfD (the reference's four files plus two for the second critic).

Both take three controls on the critic update, each None (off: the update as it was) by default: `q_bounds=(lo, hi)` clamps the
bootstrapped target-critic value, `huber_delta` shapes the TD loss, `max_grad_norm` clips each network's gradient norm before its step
(see DDPGfD's docstring; the native form: kr_critic_grad_bounded / kr_grad_sqnorm / kr_adam_step_clipped, learner_native.py).

Both take the behaviour-cloning term of Nair et al. 2018 ("Overcoming Exploration in Reinforcement Learning with Demonstrations") on the
actor update: `bc_weight` (0 = off: the update as it was) and `q_filter` (see DDPGfD's docstring; the native form: kr_bc_actor_grad).

Both take running observation normalisation, `obs_norm` (False = off: every launch and bit as it was): a running mean and standard deviation
per observation component (ObsNorm below - the specification of kr_obs_stats_update / kr_obs_normalize / kr_fold_obs_norm), every network on
the normalised state, and the rollout acting with a copy of the actor whose first layer has the affine map folded in (acting_flat).
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn
import torch.nn.functional as F


class Actor(nn.Module):
    def __init__(self, state_dim, action_dim, max_action, hidden=(400, 300)):
        super().__init__()
        self.l1 = nn.Linear(state_dim, hidden[0])
        nn.init.kaiming_uniform_(self.l1.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
        self.l2 = nn.Linear(hidden[0], hidden[1])
        nn.init.kaiming_uniform_(self.l2.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
        self.l3 = nn.Linear(hidden[1], action_dim)
        nn.init.kaiming_uniform_(self.l3.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
        self.max_action = max_action

    def forward(self, state):
        a = F.relu(self.l1(state))
        a = F.relu(self.l2(a))
        return self.max_action * torch.sigmoid(self.l3(a))


class Critic(nn.Module):
    def __init__(self, state_dim, action_dim, hidden=(400, 300)):
        super().__init__()
        self.l1 = nn.Linear(state_dim + action_dim, hidden[0])
        nn.init.kaiming_uniform_(self.l1.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
        self.l2 = nn.Linear(hidden[0], hidden[1])
        nn.init.kaiming_uniform_(self.l2.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")
        self.l3 = nn.Linear(hidden[1], 1)
        nn.init.kaiming_uniform_(self.l3.weight, a=0, mode="fan_in", nonlinearity="leaky_relu")

    def forward(self, state, action):
        q = F.relu(self.l1(torch.cat([state, action], -1)))
        q = F.relu(self.l2(q))
        return self.l3(q)


def _flatten_parameters(module: nn.Module) -> torch.Tensor:
    """Re-home the parameters of `module` as views into ONE flat fp32 buffer (returned): the soft target update is
    then a single elementwise expression per network instead of one per tensor."""
    params = list(module.parameters())
    flat = torch.cat([p.data.reshape(-1) for p in params])
    off = 0
    for p in params:
        n = p.numel()
        p.data = flat[off:off + n].view_as(p)
        off += n
    return flat


def _bounded_settings(q_bounds, huber_delta, max_grad_norm):
    """the three controls of the bounded critic update, validated; None = today's code path (not the infinite value)"""
    if q_bounds is not None:
        lo, hi = (float(x) for x in q_bounds)
        if not lo <= hi:                                   # (a NaN fails the comparison)
            raise ValueError("q_bounds=(lo, hi) needs lo <= hi, neither NaN")
        q_bounds = (lo, hi)
    if huber_delta is not None:
        huber_delta = float(huber_delta)
        if not huber_delta > 0:
            raise ValueError("huber_delta must be > 0")
    if max_grad_norm is not None:
        max_grad_norm = float(max_grad_norm)
        if not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be > 0")
    return q_bounds, huber_delta, max_grad_norm


def _bc_settings(bc_weight, q_filter):
    """the behaviour-cloning term's two settings, validated; bc_weight = 0 is today's code path"""
    bc_weight, q_filter = float(bc_weight), bool(q_filter)
    if not 0 <= bc_weight < float("inf"):                  # (a NaN fails the comparison)
        raise ValueError("bc_weight must be finite and >= 0")
    if q_filter and bc_weight == 0:
        raise ValueError("q_filter=True needs bc_weight > 0: without the behaviour-cloning term there is nothing to filter")
    return bc_weight, q_filter


def _obs_norm_settings(obs_norm, eps, freeze_after):
    """running observation normalisation's three settings, validated; obs_norm = False is today's code path.  An eps other than the default or a
    freeze_after without obs_norm=True is refused: it would silently do nothing"""
    obs_norm, eps = bool(obs_norm), float(eps)
    if not 0 < eps < float("inf"):                         # (a NaN fails the comparison)
        raise ValueError("obs_norm_eps must be finite and > 0")
    if freeze_after is not None:
        if isinstance(freeze_after, bool) or not isinstance(freeze_after, int) or freeze_after < 1:
            raise ValueError("obs_norm_freeze_after must be None or an int >= 1")
    if not obs_norm and (eps != OBS_NORM_EPS or freeze_after is not None):
        raise ValueError("obs_norm_eps / obs_norm_freeze_after need obs_norm=True")
    return obs_norm, eps, freeze_after


OBS_NORM_EPS = 1e-2        # the floor of the standard deviation: a hyper-parameter default (the folded fp32 first layer's rounding grows like
                           # |x| / sigma, and 1e-2 sits at the smallest genuine spread of an observation component, positions in metres)


class ObsNorm:
    """Running mean and standard deviation per observation component (the HER / DDPG baselines behind Nair et al. 2018), without clipping:
    the map x -> (x - mean32) * inv32 is affine and folds into a first layer, W1 ((x - m) * s) + b1 = (W1 * s) x + (b1 - (W1 * s) m).

    State: count [1], mean [S], m2 [S] in fp64 (rows so far, running mean, running sum of squared deviations) and the derived fp32 vectors
    mean32 = fp32(mean), inv32 = fp32(1 / max(sqrt(m2 / count), eps)); zeros and ones at the start: the identity.  update() takes a batch's
    rows whose weight is not 0 - two passes in fp64, batch mean then squared deviations about it, merged with Chan's parallel formula - and
    is skipped, on the device, for an all-padding batch and while `it` (updates done) has reached freeze_after.  Fixed shapes and no host
    read: it can be captured in a graph."""

    def __init__(self, dim, eps=OBS_NORM_EPS, freeze_after=None, device="cpu"):
        self.dim, self.eps, self.freeze_after = int(dim), float(eps), freeze_after
        f64 = dict(dtype=torch.float64, device=device)
        self.count, self.mean, self.m2 = torch.zeros(1, **f64), torch.zeros(dim, **f64), torch.zeros(dim, **f64)
        self.mean32, self.inv32 = torch.zeros(dim, device=device), torch.ones(dim, device=device)

    def tensors(self):
        return (self.count, self.mean, self.m2, self.mean32, self.inv32)

    @torch.no_grad()
    def update(self, x, weight=None, it=None):
        """x [rows, S]; weight [rows] or None (every row counts); it: the updates done so far, an int or a 0-d / 1-element device tensor"""
        on = torch.ones(x.shape[0], dtype=torch.bool, device=x.device) if weight is None else weight != 0
        do = on.any()
        if self.freeze_after is not None and it is not None:
            do = do & (torch.as_tensor(it, device=x.device).reshape(()) < self.freeze_after)
        col = on.unsqueeze(1)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        xd = torch.where(col, x.double(), zero)                    # (a padding row's content never enters a sum, a NaN neither)
        nb = on.sum().double()
        mb = xd.sum(0) / nb.clamp_min(1.0)
        d = torch.where(col, xd - mb, zero)
        q = (d * d).sum(0)
        na = self.count[0]
        n = (na + nb).clamp_min(1.0)
        delta = mb - self.mean
        mean = self.mean + delta * (nb / n)
        m2 = (self.m2 + q) + (delta * delta) * (na * (nb / n))
        self.mean.copy_(torch.where(do, mean, self.mean))
        self.m2.copy_(torch.where(do, m2, self.m2))
        self.count.copy_(torch.where(do, na + nb, na))
        self.derive(do)

    @torch.no_grad()
    def derive(self, do=None):
        """mean32 / inv32 from the fp64 state (where `do`, a 0-d bool tensor, when given)"""
        mean32 = self.mean.float()
        sd = torch.sqrt(self.m2 / self.count.clamp_min(1.0))
        inv32 = (1.0 / torch.where(sd > self.eps, sd, torch.full_like(sd, self.eps))).float()
        self.mean32.copy_(mean32 if do is None else torch.where(do, mean32, self.mean32))
        self.inv32.copy_(inv32 if do is None else torch.where(do, inv32, self.inv32))

    def normalize(self, x):
        """(x - mean32) * inv32 in x's dtype: an fp64 policy normalises by the same fp32-rounded numbers"""
        return (x - self.mean32.to(x.dtype)) * self.inv32.to(x.dtype)

    @torch.no_grad()
    def fold(self, W1, b1):
        """the first layer that takes raw inputs: W1 * inv32 on the first S columns, b1 - (W1 * inv32) mean32 (the sum in fp64)"""
        S = self.dim
        Wf = W1.clone()
        Wf[:, :S] = W1[:, :S] * self.inv32.to(W1.dtype)
        bf = (b1.double() - (Wf[:, :S].double() * self.mean32.double()).sum(1)).to(b1.dtype)
        return Wf, bf

    def std(self):
        """the running standard deviation per component (fp64; zeros before the first update)"""
        return torch.sqrt(self.m2 / self.count.clamp_min(1.0))


class DDPGfD:
    """q_bounds=(lo, hi): the target critic's output is clamped to [lo, hi] before it enters either target (the bootstrap, not the sum: a
    return the policy can attain lies in the range, so a correct critic is not changed).  huber_delta=d: per row and target the square
    e^2 becomes rho(e) = e^2 where not |e| > d, d (2 |e| - d) otherwise - twice the usual Huber function, d = inf is the square; its
    gradient is 2 clamp(e, -d, d).  max_grad_norm=g: torch.nn.utils.clip_grad_norm_(params, g) per network right before each
    optimizer's step (after the gradient exchange).  All three default to None = the update as it was; there is no new state.

    bc_weight=c > 0: the actor loss gains the behaviour-cloning term on the batch's demonstration rows - the window rows r >= demo_from, as
    the samplers lay a batch out: agent slots first, expert slots after -
        c * sum_{r >= demo_from} w_r sum_k f_rk |pi(s_rk) - a_rk|^2 / (sum(w) n),
    the square summed over the action's components, the normalisation that of the Q term.  f_rk = 1; with q_filter=True f_rk = 1 only
    where Q(s_rk, a_rk) > Q(s_rk, pi(s_rk)) - strict, not differentiated through, a NaN gives 0 -, both from critic 1 behind this update's
    critic step.  phase_actor then needs `action` and `demo_from`, returns the total loss and keeps the term in self.bc_loss and the
    weighted share of demonstration states that passed the filter in self.bc_pass (0-d tensors, no host sync).  bc_weight=0 (the default)
    is the update as it was in every bit; there is no new state and nothing new in checkpoints.

    obs_norm=True: running observation normalisation (ObsNorm; obs_norm_eps the floor of the standard deviation, obs_norm_freeze_after=N: the
    statistics stop after N updates).  Once per update, before any network pass, the statistics take the batch's window-first states
    state[:, 0] whose weight is not 0; then every network - actor, critics, all targets - sees (x - mean32) * inv32 of the S state columns
    (the critic's action columns stay).  The phases keep taking raw states.  Whatever acts on raw observations goes through act() - or, for
    the rollout kernels, through acting_flat() / acting_layers(): a copy of the actor with the map folded into its first layer, rewritten
    after every update.  One more checkpoint file, <prefix>_obs_norm.  Not with a process group of more than one rank: per-rank statistics
    would give the ranks different functions under shared weights.  obs_norm=False (the default): nothing of this exists."""

    def __init__(self, state_dim=82, action_dim=4, max_action=0.8, n=5, discount=0.995, tau=0.0005, batch_size=64,
                 hidden=(400, 300), device="cpu", process_group=None, capturable=False, q_bounds=None, huber_delta=None, max_grad_norm=None,
                 bc_weight=0.0, q_filter=False, obs_norm=False, obs_norm_eps=OBS_NORM_EPS, obs_norm_freeze_after=None):
        self.q_bounds, self.huber_delta, self.max_grad_norm = _bounded_settings(q_bounds, huber_delta, max_grad_norm)
        self.bc_weight, self.q_filter = _bc_settings(bc_weight, q_filter)
        obs_norm, obs_norm_eps, obs_norm_freeze_after = _obs_norm_settings(obs_norm, obs_norm_eps, obs_norm_freeze_after)
        if obs_norm:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
                raise ValueError("obs_norm=True keeps its statistics per rank: not with a process group of more than one rank")
        self.device = torch.device(device)
        self.obs_norm = ObsNorm(state_dim, obs_norm_eps, obs_norm_freeze_after, self.device) if obs_norm else None
        self._acting = self._acting_views = None             # obs_norm: the actor with the normalisation folded into its first layer
        self.bc_loss, self.bc_pass = torch.zeros((), device=self.device), torch.zeros((), device=self.device)
        self.actor = Actor(state_dim, action_dim, max_action, hidden).to(self.device)
        self.actor_target = copy.deepcopy(self.actor)
        self._flat_params = {}
        # capturable: optimizer state and the update counter live on the device, so that a whole update can be
        # captured in a HIP graph (pipeline.GraphedTrainer); the arithmetic is the same
        self.capturable = bool(capturable)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=1e-4, capturable=self.capturable)
        self.critic = Critic(state_dim, action_dim, hidden).to(self.device)
        self.critic_target = copy.deepcopy(self.critic)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), weight_decay=1e-4, capturable=self.capturable)
        self._it_dev = torch.zeros((), dtype=torch.long, device=self.device)
        for name in ("actor", "actor_target", "critic", "critic_target"):
            self._flat_params[name] = _flatten_parameters(getattr(self, name))
        self.discount, self.tau, self.n = discount, tau, n
        self._disc = torch.tensor([discount ** i for i in range(n)], dtype=torch.float32, device=self.device)
        self.network_repl_freq = 10
        self.total_it = 0
        self.batch_size = batch_size
        self.max_action = max_action
        self.process_group = process_group
        self._flat = None
        self._native = None          # learner_native.NativeDDPGfDUpdate attached to this policy (keeps its own flat Adam state)
        self.refresh_acting()

    # -- inference ------------------------------------------------------------------------------
    @torch.no_grad()
    def select_action(self, state):
        """state: [..., 82] tensor/array -> actions [..., 4] (stays on the device for tensors)"""
        if not torch.is_tensor(state):
            s = torch.as_tensor(state, dtype=torch.float32, device=self.device).reshape(1, -1)
            return self.act(s).cpu().numpy().flatten()
        return self.act(state)

    def _norm(self, state):
        """what the networks see of raw states (obs_norm; else the states themselves)"""
        return state if self.obs_norm is None else self.obs_norm.normalize(state)

    def act(self, state):
        """the actor on RAW observations: the one place that evaluates it on them (select_action, the rollout's torch paths, evaluation)"""
        return self.actor(self._norm(state))

    def acting_flat(self):
        """the flat parameter buffer the rollout acts with, in the actor's own layout: the actor's itself, or with obs_norm the copy whose
        first layer has the normalisation folded in (refresh_acting; the native learner rewrites it with kr_fold_obs_norm every update)"""
        return self._flat_params["actor"] if self.obs_norm is None else self._acting_buffer()

    def acting_layers(self):
        """[(weight, bias)] x 3 of acting_flat(), as mlp.layers_of gives the actor's"""
        if self.obs_norm is None:
            return [(getattr(self.actor, k).weight.data, getattr(self.actor, k).bias.data) for k in ("l1", "l2", "l3")]
        self._acting_buffer()
        return self._acting_views

    def _acting_buffer(self):
        flat = self._flat_params["actor"]
        if self._acting is None or self._acting.shape != flat.shape or self._acting.dtype != flat.dtype or self._acting.device != flat.device:
            self._acting = flat.clone()
            views, off = [], 0
            for k in ("l1", "l2", "l3"):
                lin = getattr(self.actor, k)
                w = self._acting[off:off + lin.weight.numel()].view_as(lin.weight)
                off += lin.weight.numel()
                b = self._acting[off:off + lin.bias.numel()].view_as(lin.bias)
                off += lin.bias.numel()
                views.append((w, b))
            self._acting_views = views
        return self._acting

    @torch.no_grad()
    def refresh_acting(self):
        """obs_norm: acting_flat() <- fold(the actor as it is, the statistics as they are); the torch form of kr_fold_obs_norm"""
        if self.obs_norm is None:
            return
        self._acting_buffer().copy_(self._flat_params["actor"])
        (w1, b1), _, _ = self._acting_views
        wf, bf = self.obs_norm.fold(self.actor.l1.weight.data, self.actor.l1.bias.data)
        w1.copy_(wf)
        b1.copy_(bf)

    # -- gradient exchange: one all-reduce over a flat buffer holding both networks ---
    def _allreduce_grads(self, params):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(self.process_group)
        if world == 1:
            return
        grads = [p.grad for p in params]
        flat = torch.cat([g.reshape(-1) for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.process_group)
        flat.div_(world)
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()

    # -- update ---------------------------------------------------------------------------------
    def train_on_batch(self, state, action, next_state, reward, weight=None, demo_from=None):
        """One DDPGfD update on already-sampled n-step windows: state/next_state [R, n, 82],
        action [R, n, 4], reward [R, n].  `weight` [R] (optional, 0/1) masks padding rows so that
        fixed-shape device batches keep the reference's per-row means.  Returns the four losses
        (actor, critic, critic_L1, critic_LN) as 0-d tensors (no host sync).  demo_from (needed with bc_weight > 0): the
        rows r >= demo_from are demonstration rows.

        The update is three phases with a gradient exchange after the first two (`phase_critic`,
        `phase_actor`, `phase_targets`); pipeline.GraphedTrainer captures the phases in HIP graphs and runs the
        exchanges between them."""
        losses_c = self.phase_critic(state, action, next_state, reward, weight)
        self._allreduce_grads(list(self.critic.parameters()))
        actor_loss = self.phase_actor(state, weight, action, demo_from)
        self._allreduce_grads(list(self.actor.parameters()))
        self.phase_targets()
        return (actor_loss,) + losses_c

    @staticmethod
    def _mean(x, per_row, weight):
        if weight is None:
            return x.mean()
        w = weight.view(-1, *([1] * (x.dim() - 1)))
        return (x * w).sum() / (w.sum().clamp_min(1.0) * per_row)      # 0 / 1 weights: exact unless the batch is all padding

    def _bound(self, tq):
        """the bootstrapped value the targets take (q_bounds)"""
        return tq if self.q_bounds is None else tq.clamp(self.q_bounds[0], self.q_bounds[1])

    def _rho(self, e):
        """the TD loss per row and target (huber_delta); a NaN error takes the square branch and stays NaN"""
        if self.huber_delta is None:
            return e ** 2
        # c (2 e - c) with c = clamp(e, -d, d): e^2 inside, d (2 |e| - d) outside, gradient 2 c - and no inf * 0 in the backward pass
        # of a branch that is not taken, so that d = inf is the square in every bit
        c = e.clamp(-self.huber_delta, self.huber_delta)
        return c * (2 * e - c)

    def _clip(self, module):
        """the global gradient-norm clip of one network, right before its optimizer's step (max_grad_norm)"""
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(module.parameters(), self.max_grad_norm)

    def _bootstrap(self, nx, target_noise=None):
        """the target critic's value of the target actor's action at the states nx (before q_bounds)"""
        if target_noise is not None:
            raise ValueError("DDPGfD has no target smoothing: target_noise belongs to TD3fD")
        return self.critic_target(nx, self.actor_target(nx))

    def _critics(self):
        """the (critic, optimizer) pairs phase_critic trains on the common targets"""
        return ((self.critic, self.critic_optimizer),)

    def phase_critic(self, state, action, next_state, reward, weight=None, target_noise=None):
        """targets + critic loss + backward (DDPGfD.py:256-330).  Returns (critic, L1, LN) losses, per critic of _critics().  obs_norm: the
        statistics take state[:, 0] first - this phase opens the update -, then the networks see the normalised states."""
        if self.obs_norm is not None:
            self.obs_norm.update(state[:, 0], weight, self._it_dev if self.capturable else self.total_it)
            state, next_state = self._norm(state), self._norm(next_state)
        reward = reward.unsqueeze(-1)
        with torch.no_grad():
            # both target evaluations (1-step: next_state[:, 0], n-step: next_state[:, -1]) in one pass of the target nets
            R = reward.shape[0]
            nx = torch.cat([next_state[:, 0], next_state[:, -1]], 0)
            tq = self._bound(self._bootstrap(nx, target_noise))
            target_Q = reward[:, 0] + self.discount * tq[:R]
            n_step_return = (reward.squeeze(-1) * self._disc).sum(1)
            target_QN = (n_step_return + (self.discount ** self.n) * tq[R:].squeeze(-1)).unsqueeze(-1)
        out, total = (), None
        for critic, _ in self._critics():
            current_Q = critic(state[:, 0], action[:, 0])
            L1 = self._mean(self._rho(current_Q - target_Q), 1, weight)
            LN = self._mean(self._rho(current_Q - target_QN), 1, weight)
            loss = L1 + 0.5 * LN
            total = loss if total is None else total + loss
            out += (loss.detach(), L1.detach(), LN.detach())
        for _, optimizer in self._critics():
            optimizer.zero_grad()
        total.backward()
        return out

    def _bc_term(self, state, action, pi, q_pi, weight, demo_from):
        """the behaviour-cloning term of the actor loss on the rows r >= demo_from (see the class docstring) and the weighted share of
        their states that passed the filter; the critic is critic 1 as phase_actor holds it"""
        R, n, d = state.shape[0], state.shape[1], int(demo_from)
        sq = ((pi[d:] - action[d:]) ** 2).sum(-1)                        # [R - d, n]
        if self.q_filter:
            with torch.no_grad():
                f = (self.critic(state[d:], action[d:]) > q_pi[d:]).squeeze(-1).to(sq.dtype)      # strict; a NaN compares false
        else:
            f = torch.ones_like(sq)
        w = torch.ones(R, dtype=sq.dtype, device=sq.device) if weight is None else weight
        wd = w[d:].unsqueeze(-1)
        bc = self.bc_weight * (sq * f * wd).sum() / (w.sum().clamp_min(1.0) * n)
        share = (f * wd).sum() / (wd.sum() * n).clamp_min(torch.finfo(sq.dtype).tiny)
        return bc, share.detach()

    def phase_actor(self, state, weight=None, action=None, demo_from=None):
        """critic step, then actor loss + backward (DDPGfD.py:331-352); with bc_weight > 0 the loss has the behaviour-cloning term on the
        rows r >= demo_from of `action` (self.bc_loss, self.bc_pass)"""
        state = self._norm(state)
        if self.bc_weight > 0:
            return self._phase_actor_bc(state, weight, action, demo_from)
        self._clip(self.critic)
        self.critic_optimizer.step()
        # the critic is only a differentiable function here: no weight gradients for it (the reference computes and
        # discards them)
        for p in self.critic.parameters():
            p.requires_grad_(False)
        actor_loss = -self._mean(self.critic(state, self.actor(state)), state.shape[1], weight)
        self.actor_optimizer.zero_grad()
        actor_loss.backward()
        for p in self.critic.parameters():
            p.requires_grad_(True)
        return actor_loss.detach()

    def _phase_actor_bc(self, state, weight, action, demo_from):
        if action is None or demo_from is None:
            raise ValueError("bc_weight > 0: the actor phase needs the batch's actions and demo_from, the first demonstration row")
        if not 0 <= int(demo_from) <= state.shape[0]:
            raise ValueError("demo_from must lie in [0, rows]")
        self._clip(self.critic)
        self.critic_optimizer.step()
        for p in self.critic.parameters():
            p.requires_grad_(False)
        pi = self.actor(state)
        q_pi = self.critic(state, pi)
        bc, share = self._bc_term(state, action, pi, q_pi.detach(), weight, demo_from)
        actor_loss = -self._mean(q_pi, state.shape[1], weight) + bc
        self.actor_optimizer.zero_grad()
        actor_loss.backward()
        for p in self.critic.parameters():
            p.requires_grad_(True)
        self.bc_loss, self.bc_pass = bc.detach(), share
        return actor_loss.detach()

    def phase_targets(self):
        """actor step + soft target update on every 10th call (DDPGfD.py:353-366)"""
        self._clip(self.actor)
        self.actor_optimizer.step()
        self.total_it += 1
        fp = self._flat_params
        pairs = ((fp["critic"], fp["critic_target"]), (fp["actor"], fp["actor_target"]))
        with torch.no_grad():
            if self.capturable:
                # device-side gate: tau on every network_repl_freq-th call, else 0 (same arithmetic when it fires)
                self._it_dev += 1
                fire = self._it_dev % self.network_repl_freq == 0
                for p, tp in pairs:
                    tp.copy_(torch.where(fire, self.tau * p + (1 - self.tau) * tp, tp))
            elif self.total_it % self.network_repl_freq == 0:
                for p, tp in pairs:
                    tp.copy_(self.tau * p + (1 - self.tau) * tp)
        self.refresh_acting()

    def train_batch(self, episode_step, expert_replay_buffer, replay_buffer, num_trajectories=5, prob=0.3):
        """Reference signature (DDPGfD.py:219): samples agent (1-prob) / expert (prob) episodes from
        buffers exposing sample_batch_nstep(batch_size) and runs one update.  Returns floats."""
        if replay_buffer is not None and expert_replay_buffer is None:
            batch = replay_buffer.sample_batch_nstep(self.batch_size)
        elif replay_buffer is None and expert_replay_buffer is not None:
            batch = expert_replay_buffer.sample_batch_nstep(self.batch_size)
        else:
            agent_bs = int(self.batch_size * (1 - prob))
            ag = replay_buffer.sample_batch_nstep(agent_bs)
            ex = expert_replay_buffer.sample_batch_nstep(self.batch_size - agent_bs)
            batch = tuple(torch.cat((a, e), 0) for a, e in zip(ag, ex))
            demo_from = ag[0].shape[0]                     # agent rows first, expert rows after
        state, action, next_state, reward = (t.to(self.device) for t in batch[:4])
        weight = batch[5].to(self.device) if len(batch) > 5 else None
        if replay_buffer is None or expert_replay_buffer is None:
            demo_from = 0 if replay_buffer is None else state.shape[0]
        return tuple(x.item() for x in self.train_on_batch(state, action, next_state, reward, weight, demo_from=demo_from))

    # -- checkpoints: the reference's four files (DDPGfD.py:371-382) ---------------------------------
    def save(self, filename):
        if self._native is not None:
            self._native.export_optimizer_state()     # the native learner's Adam moments / step -> the torch optimizers' state
        torch.save(self.critic.state_dict(), filename + "_critic")
        torch.save(self.critic_optimizer.state_dict(), filename + "_critic_optimizer")
        torch.save(self.actor.state_dict(), filename + "_actor")
        torch.save(self.actor_optimizer.state_dict(), filename + "_actor_optimizer")
        if self.obs_norm is not None:
            on = self.obs_norm
            torch.save({"count": on.count.cpu(), "mean": on.mean.cpu(), "m2": on.m2.cpu(), "eps": on.eps, "freeze_after": on.freeze_after},
                       filename + "_obs_norm")

    def load(self, filename, weights_only=True, sync_targets=False):
        """Like the reference, loading leaves the target networks untouched (DDPGfD.py:378-382);
        sync_targets=True copies the loaded weights into them.  obs_norm: <prefix>_obs_norm must be there (the weights mean nothing without
        the statistics they were trained on) and its eps / freeze_after are adopted; without obs_norm the file is neither needed nor read."""
        import os
        if self.obs_norm is not None and not os.path.exists(filename + "_obs_norm"):
            raise FileNotFoundError(f"{filename}_obs_norm is missing: a policy with obs_norm=True needs the statistics its weights were trained on")
        self.critic.load_state_dict(torch.load(filename + "_critic", map_location=self.device, weights_only=weights_only))
        self.actor.load_state_dict(torch.load(filename + "_actor", map_location=self.device, weights_only=weights_only))
        if os.path.exists(filename + "_critic_optimizer"):
            self.critic_optimizer.load_state_dict(torch.load(filename + "_critic_optimizer", map_location=self.device, weights_only=weights_only))
        if os.path.exists(filename + "_actor_optimizer"):
            self.actor_optimizer.load_state_dict(torch.load(filename + "_actor_optimizer", map_location=self.device, weights_only=weights_only))
        if sync_targets:
            self.critic_target.load_state_dict(self.critic.state_dict())
            self.actor_target.load_state_dict(self.actor.state_dict())
        self._load_extra(filename, weights_only, sync_targets)
        if self.obs_norm is not None:
            on, st = self.obs_norm, torch.load(filename + "_obs_norm", map_location=self.device, weights_only=weights_only)
            if tuple(st["mean"].shape) != (on.dim,):
                raise ValueError(f"{filename}_obs_norm holds statistics of {tuple(st['mean'].shape)} components, the policy has {on.dim}")
            on.count.copy_(st["count"]); on.mean.copy_(st["mean"]); on.m2.copy_(st["m2"])
            on.eps, on.freeze_after = _obs_norm_settings(True, st["eps"], st["freeze_after"])[1:]
            on.derive()
        if self._native is not None:
            self._native.import_optimizer_state()     # ... and back: the native learner continues from the loaded Adam state
        self.refresh_acting()

    def _load_extra(self, filename, weights_only, sync_targets):
        """files beyond the reference's four (TD3fD's second critic); they are ignored here, so a TD3fD checkpoint loads into a DDPGfD"""


class TD3fD(DDPGfD):
    """DDPGfD with TD3's three parts (Fujimoto et al. 2018; the reference group's `Old Code/TD3.py`) on the n-step / demonstration update:

    * twin critics: `critic2` / `critic2_target` (independently initialised) and `critic2_optimizer` (the critic's hyper-parameters); both
      targets (1-step and n-step) bootstrap from min(critic_target, critic2_target);
    * smoothed target actions: clamp(actor_target(s') + clamp(policy_noise * z, -noise_clip, noise_clip), 0, max_action), z ~ N(0, 1).
      TD3's published 0.2 / 0.5 are stated for a unit action half-range; this actor's half-range is max_action / 2, hence the defaults
      policy_noise = 0.1 * max_action and noise_clip = 0.25 * max_action;
    * a delayed actor: its optimizer steps on the updates with it % policy_freq == 0 only (its own step count is it / policy_freq); the
      gradient of the other updates is computed and dropped.  The soft update of the three target networks keeps its
      network_repl_freq gate on `it`.

    The actor loss goes through critic 1 only, as in TD3.  These autograd phases are the specification of the native form
    (learner_native.NativeDDPGfDUpdate takes a TD3fD policy).  Checkpoints: the reference's four files plus `<prefix>_critic2` and
    `<prefix>_critic2_optimizer`."""

    def __init__(self, state_dim=82, action_dim=4, max_action=0.8, n=5, discount=0.995, tau=0.0005, batch_size=64, hidden=(400, 300),
                 device="cpu", process_group=None, capturable=False, policy_noise=None, noise_clip=None, policy_freq=2, q_bounds=None,
                 huber_delta=None, max_grad_norm=None, bc_weight=0.0, q_filter=False, obs_norm=False, obs_norm_eps=OBS_NORM_EPS, obs_norm_freeze_after=None):
        super().__init__(state_dim, action_dim, max_action, n, discount, tau, batch_size, hidden, device, process_group, capturable,
                         q_bounds=q_bounds, huber_delta=huber_delta, max_grad_norm=max_grad_norm, bc_weight=bc_weight, q_filter=q_filter,
                         obs_norm=obs_norm, obs_norm_eps=obs_norm_eps, obs_norm_freeze_after=obs_norm_freeze_after)
        self.critic2 = Critic(state_dim, action_dim, hidden).to(self.device)
        self.critic2_target = copy.deepcopy(self.critic2)
        self.critic2_optimizer = torch.optim.Adam(self.critic2.parameters(), weight_decay=1e-4, capturable=self.capturable)
        for name in ("critic2", "critic2_target"):
            self._flat_params[name] = _flatten_parameters(getattr(self, name))
        self.policy_noise = 0.1 * max_action if policy_noise is None else float(policy_noise)
        self.noise_clip = 0.25 * max_action if noise_clip is None else float(noise_clip)
        self.policy_freq = int(policy_freq)
        if not (self.policy_noise >= 0 and self.noise_clip >= 0 and self.policy_freq >= 1):
            raise ValueError("TD3fD: policy_noise and noise_clip must be >= 0, policy_freq >= 1")

    def train_on_batch(self, state, action, next_state, reward, weight=None, target_noise=None, demo_from=None):
        """As DDPGfD.train_on_batch; returns (actor, critic, critic_L1, critic_LN, critic2, critic2_L1, critic2_LN).  target_noise: the
        N(0, 1) draws of the target smoothing, [2R, 4] (None: torch.randn)."""
        losses_c = self.phase_critic(state, action, next_state, reward, weight, target_noise)
        self._allreduce_grads(list(self.critic.parameters()) + list(self.critic2.parameters()))
        actor_loss = self.phase_actor(state, weight, action, demo_from)
        self._allreduce_grads(list(self.actor.parameters()))
        self.phase_targets()
        return (actor_loss,) + losses_c

    # DDPGfD.phase_critic with these two: smoothed target actions, the twin targets' minimum (q_bounds clamps after it), both critics'
    # losses summed before one backward().  It returns (critic, L1, LN) of critic 1, then of critic 2.
    def _bootstrap(self, nx, target_noise=None):
        a = self.actor_target(nx)
        z = torch.randn_like(a) if target_noise is None else target_noise
        ta = (a + (self.policy_noise * z).clamp(-self.noise_clip, self.noise_clip)).clamp(0, self.max_action)
        return torch.min(self.critic_target(nx, ta), self.critic2_target(nx, ta))

    def _critics(self):
        return ((self.critic, self.critic_optimizer), (self.critic2, self.critic2_optimizer))

    def phase_actor(self, state, weight=None, action=None, demo_from=None):
        """both critics' steps, then the actor loss through critic 1 (the behaviour-cloning term and its filter too) + backward"""
        if self.bc_weight > 0 and (action is None or demo_from is None or not 0 <= int(demo_from) <= state.shape[0]):
            raise ValueError("bc_weight > 0: the actor phase needs the batch's actions and demo_from, the first demonstration row, in [0, rows]")
        self._clip(self.critic2)
        self.critic2_optimizer.step()
        return super().phase_actor(state, weight, action, demo_from)

    def phase_targets(self):
        """the actor's step on every policy_freq-th call + soft update of the three target networks on every 10th call"""
        self.total_it += 1
        fp = self._flat_params
        pairs = ((fp["critic"], fp["critic_target"]), (fp["critic2"], fp["critic2_target"]), (fp["actor"], fp["actor_target"]))
        if self.capturable:
            # device-side gates: the step is taken and then undone where the gate is closed (same arithmetic where it is open)
            self._it_dev += 1
            opt, flat = self.actor_optimizer, fp["actor"]
            step_now = self._it_dev % self.policy_freq == 0
            params = [p for p in opt.param_groups[0]["params"] if p.grad is not None]
            keys = ("step", "exp_avg", "exp_avg_sq")
            before = [{k: opt.state[p][k].clone() for k in keys} if opt.state.get(p) else None for p in params]
            flat_before = flat.clone()
            self._clip(self.actor)                 # (before the step that the gate may undo)
            opt.step()
            with torch.no_grad():
                flat.copy_(torch.where(step_now, flat, flat_before))
                for p, old in zip(params, before):
                    for k in keys:
                        cur = opt.state[p][k]
                        cur.copy_(torch.where(step_now, cur, torch.zeros_like(cur) if old is None else old[k]))
                fire = self._it_dev % self.network_repl_freq == 0
                for p, tp in pairs:
                    tp.copy_(torch.where(fire, self.tau * p + (1 - self.tau) * tp, tp))
            self.refresh_acting()
            return
        if self.total_it % self.policy_freq == 0:
            self._clip(self.actor)
            self.actor_optimizer.step()
        if self.total_it % self.network_repl_freq == 0:
            with torch.no_grad():
                for p, tp in pairs:
                    tp.copy_(self.tau * p + (1 - self.tau) * tp)
        self.refresh_acting()

    def save(self, filename):
        super().save(filename)
        torch.save(self.critic2.state_dict(), filename + "_critic2")
        torch.save(self.critic2_optimizer.state_dict(), filename + "_critic2_optimizer")

    def _load_extra(self, filename, weights_only, sync_targets):
        """a four-file checkpoint leaves critic2 as it is"""
        import os
        if os.path.exists(filename + "_critic2"):
            self.critic2.load_state_dict(torch.load(filename + "_critic2", map_location=self.device, weights_only=weights_only))
        if os.path.exists(filename + "_critic2_optimizer"):
            self.critic2_optimizer.load_state_dict(torch.load(filename + "_critic2_optimizer", map_location=self.device, weights_only=weights_only))
        if sync_targets:
            self.critic2_target.load_state_dict(self.critic2.state_dict())
