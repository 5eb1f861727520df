"""The TD3 learner behind the reference's class API (base/core/td3.py:17-198): `Critic`, and `TD3` with `.actor`, `.actor_target`,
`.critic`, `.critic_target`, `.buffer`, `.critical_buffer`, `update_parameters(batch, iteration, champion_policy)`.

`update_parameters` is one eager update, as the reference runs it.  `train` is what Agent.train_rl (base/core/agent.py:155-186) does
with it -- one update per frame of the generation, minibatches sampled from the shared replay buffer -- as ONE kernel launch
(serl_td3_train, include/serl_amd.h): the host draws the minibatch slots from python's `random` stream and the noise from a torch CPU
generator in the order a CPU run of the reference consumes them, the device does the rest.  Without a GPU, or for a shape the kernel
is not compiled for, `train` loops `update_parameters` over the same draws.

`train(draws='device', seed=...)` takes no draw on the host at all: serl_td3_train_rng draws the slots and both kinds of noise inside the
kernel from the counter-based generator of csrc/serl_rng.h, as a function of (seed, learner, iteration), and `td3_draws` writes the same
draws out as tables (serl_td3_rng_fill) for a replay on the table path.

`TD3Group(learners).train(replays, n_updates, iteration0=..., seed=...)` runs the updates of several independent learners of one network
shape -- seeds, hyper-parameter settings -- as ONE launch (serl_td3_train_group), each learner where its own train(draws='device') would
put it.  Minibatches of 129 .. 512 rows run on serl_td3_train_group_big, one workgroup per learner walking the chunks of 128 samples, and
`chunks='parallel'` puts every chunk of every learner on a workgroup of its own (serl_td3_train_group_wide), as TD3.train's `chunks` does
for one learner.
"""
import ctypes
import random
import numpy as np
import torch
import torch.nn as nn
from torch.nn import functional as F
from torch.optim import Adam
from . import replay as _replay
from .actor import Actor, LayerNorm, _activation, pack_actor, unpack_into, pack_critic, unpack_critic, ACTIVATION_IDS

MAX_GRAD_NORM = 10.0            # td3.py:13
CRITIC_HIDDEN = 64              # td3.py:24
CAPS = {'lambda_s': 0.5, 'lambda_t': 0.1, 'eps_sd': 0.05}          # td3.py:115-120
# `train` takes the fused path by default because it was measured faster than the eager float32 loop on the same MI355X at the default
# shape (hidden 72, 3 layers, minibatch 86, CAPS on): tools/bench_td3.py, profiles/td3_fused_timing.json.
FUSED_DEFAULT = True
# train(dense=...): the entry point of the library and what last_path reports.  'valu' is the default: 'mfma' gives the same bits and is
# opt-in until profiles/td3_mfma_timing.json decides otherwise.
DENSE = {'valu': ('serl_td3_train', 'fused'), 'mfma': ('serl_td3_train_mfma', 'fused-mfma')}
# train(draws=...): 'host' = slots from `rng`, noise from `generator`, uploaded as tables (the default; profiles/td3_rng_timing.json
# holds the measurements a later change decides from); 'device' = serl_td3_train_rng, last_path 'fused-rng' / 'fused-mfma-rng'.
DRAWS = ('host', 'device')
# minibatches of more rows than serl_td3_train takes (up to 512) run on serl_td3_train_big when asked for by name -- fused=True,
# dense='mfma' or draws='device'; last_path gains '-big' after the dense flavour.  fused=None keeps the eager loop for them.
FUSED_MAX_BATCH = 128
# train(chunks=...): 'serial' = as above (the default); 'parallel' = serl_td3_train_wide, the chunks of 128 samples of a minibatch of up to
# 512 rows on workgroups of their own, bit for bit serl_td3_train_big's result; last_path 'fused-wide' / 'fused-mfma-wide' (+ '-rng').
CHUNKS = ('serial', 'parallel')


class _QNet(nn.Module):
    """one of the twins: Linear(S + A, 64) LayerNorm act, Linear(64, 64) LayerNorm act, Linear(64, 1)"""

    def __init__(self, n_in, activation):
        super().__init__()
        self.l1 = nn.Linear(n_in, CRITIC_HIDDEN)
        self.ln1 = LayerNorm(CRITIC_HIDDEN)
        self.l2 = nn.Linear(CRITIC_HIDDEN, CRITIC_HIDDEN)
        self.ln2 = LayerNorm(CRITIC_HIDDEN)
        self.out = nn.Linear(CRITIC_HIDDEN, 1)
        self.act = _activation(activation)
        with torch.no_grad():                   # the output layer starts small (td3.py:46-47)
            self.out.weight.mul_(0.1)
            self.out.bias.mul_(0.1)

    def forward(self, x):
        h = self.act(self.ln1(self.l1(x)))
        h = self.act(self.ln2(self.l2(h)))
        return self.out(h)


class Critic(nn.Module):
    """Twin Q-networks on (state, action) -> (q1, q2), the callable `ssne.SSNE(critic=...)` expects.  Only what the reference's Critic
    trains: its two BatchNorm layers are never called and never get a gradient, so they are left out; parameters() walks critic 1, then
    critic 2, in the order of the packed row (actor.pack_critic)."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        n_in = args.state_dim + args.action_dim
        self.q1 = _QNet(n_in, args.activation_actor)
        self.q2 = _QNet(n_in, args.activation_actor)
        self.to(getattr(args, 'device', 'cpu'))

    def forward(self, state, action):
        x = torch.cat((state, action), 1)
        return self.q1(x), self.q2(x)


def critic_param_count(state_dim, action_dim):
    H = CRITIC_HIDDEN
    return 2 * (H * (state_dim + action_dim) + 3 * H + H * H + 3 * H + H + 1)


def _hard_update(target, source):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.copy_(s)


def _soft_update(target, source, tau):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.copy_(t * (1.0 - tau) + s * tau)


def _pack_adam(optim, params):
    """(first moments, second moments, steps taken) of a torch Adam over `params`, as packed f32 rows"""
    m, v, step = [], [], 0
    for p in params:
        st = optim.state.get(p, {})
        m.append(st['exp_avg'].detach().reshape(-1) if 'exp_avg' in st else torch.zeros(p.numel()))
        v.append(st['exp_avg_sq'].detach().reshape(-1) if 'exp_avg_sq' in st else torch.zeros(p.numel()))
        if 'step' in st:
            step = int(st['step'])
    return torch.cat(m).to(torch.float32).cpu(), torch.cat(v).to(torch.float32).cpu(), step


def _unpack_adam(optim, params, m, v, step):
    off = 0
    m, v = m.detach().cpu(), v.detach().cpu()
    for p in params:
        n = p.numel()
        optim.state[p] = {'step': torch.tensor(float(step)),
                          'exp_avg': m[off:off + n].view(p.shape).to(device=p.device, dtype=p.dtype).clone(),
                          'exp_avg_sq': v[off:off + n].view(p.shape).to(device=p.device, dtype=p.dtype).clone()}
        off += n


# ---- what TD3.train and TD3Group.train share: a launch of K learners (K = 1 for TD3.train) -----------------------------------------------
ROWS = ('actor', 'actor_target', 'actor_m', 'actor_v', 'critic', 'critic_target', 'critic_m', 'critic_v')
_NAN = {'PG_obj': float('nan'), 'TD_loss': float('nan')}


def _names(dense, big=False, rng=False, group=False, wide=False):
    """-> (the library's entry point, what last_path reports) of a fused launch"""
    entry = (('serl_td3_train_group_wide' if wide else 'serl_td3_train_group_big' if big else 'serl_td3_train_group') if group else
             'serl_td3_train_wide' if wide else 'serl_td3_train_big' if big else 'serl_td3_train_rng' if rng else DENSE[dense][0])
    return entry, (DENSE[dense][1] + ('-wide' if wide else '-big' if big else '') + ('-group' if group else '') +
                   ('-rng' if rng or group else ''))


def _pack(learners, dev):
    """-> (rows, steps): the eight packed f32 rows of the learners, [K, parameters] each on `dev`, and the Adam steps taken, i32 [K, 2]
    (critic, actor)"""
    packed, steps = {k: [] for k in ROWS}, []
    for t in learners:
        am, av, astep = _pack_adam(t.actor_optim, list(t.actor.parameters()))
        cm, cv, cstep = _pack_adam(t.critic_optim, list(t.critic.parameters()))
        for k, v in zip(ROWS, (pack_actor(t.actor), pack_actor(t.actor_target), am, av,
                               pack_critic(t.critic), pack_critic(t.critic_target), cm, cv)):
            packed[k].append(v.detach().to(torch.float32).cpu())
        steps.append([cstep, astep])
    return {k: torch.stack(v).contiguous().to(dev) for k, v in packed.items()}, torch.tensor(steps, dtype=torch.int32, device=dev)


def _unpack(t, rows, steps, i):
    """row i of what _pack made, after a launch, back into learner t; steps: [K][2] integers.  The actor's optimiser is only written
    once it has stepped (as the eager loop leaves it untouched until the first actor update)."""
    unpack_into(t.actor, rows['actor'][i])
    unpack_into(t.actor_target, rows['actor_target'][i])
    unpack_critic(t.critic, rows['critic'][i])
    unpack_critic(t.critic_target, rows['critic_target'][i])
    cstep, astep = (int(x) for x in steps[i])
    _unpack_adam(t.critic_optim, list(t.critic.parameters()), rows['critic_m'][i], rows['critic_v'][i], cstep)
    if astep:
        _unpack_adam(t.actor_optim, list(t.actor.parameters()), rows['actor_m'][i], rows['actor_v'][i], astep)


def _learner_fields(t, replay, iteration0, update_actor_target):
    """what is a learner's own in a launch, under the names Td3Desc (one learner's values for the launch) and Td3LearnerRow (a group's
    row) share"""
    a, c = t.args, t.caps_dict or {'lambda_s': 0.0, 'lambda_t': 0.0, 'eps_sd': 0.0}
    return dict(capacity=replay.capacity, iteration0=int(iteration0), policy_update_freq=int(a.policy_update_freq),
                update_actor_target=int(bool(update_actor_target)), lr=a.lr, gamma=a.gamma, tau=a.tau, noise_sd=a.noise_sd,
                noise_clip=a.noise_clip, lambda_s=c['lambda_s'], lambda_t=c['lambda_t'], eps_sd=c['eps_sd'])


def _describe(args, n, rows, steps, td, pg, work, **per_launch):
    """the Td3Desc of a launch of the K learners packed in `rows` (network shape and minibatch from `args`), at most n updates each, losses
    to td / pg [K, n], workspace `work`; per_launch: the fields only some entry points read (_learner_fields, the ring, the tables)"""
    from . import _capi
    ptr = lambda x: x.data_ptr()
    return _capi.Td3Desc(state_dim=args.state_dim, action_dim=args.action_dim, hidden=args.hidden_size, num_layers=args.num_layers,
                         activation=ACTIVATION_IDS[args.activation_actor.lower()], n_learners=rows['actor'].shape[0],
                         batch=int(args.batch_size), n_updates=n, max_grad_norm=MAX_GRAD_NORM,
                         actor_stride=rows['actor'].stride(0), critic_stride=rows['critic'].stride(0), **{k: ptr(rows[k]) for k in ROWS},
                         adam_steps=ptr(steps), td_loss=ptr(td), pg_loss=ptr(pg), loss_stride=n, work=ptr(work),
                         work_bytes=work.numel() * work.element_size(), **per_launch)


def _outputs(L, args, K, n, big, dev, wide=False):
    """-> (td zeros [K, n], pg NaN [K, n], the workspace of the launch) on `dev`"""
    size = L.serl_td3_wide_work_bytes if wide else L.serl_td3_big_work_bytes if big else L.serl_td3_work_bytes
    wb = int(size(K, args.state_dim, args.action_dim, args.hidden_size, args.num_layers, int(args.batch_size)))
    return (torch.zeros(K, n, dtype=torch.float32, device=dev), torch.full((K, n), float('nan'), dtype=torch.float32, device=dev),
            torch.empty(wb // 4, dtype=torch.float32, device=dev))


def _reduce(td, pg):
    """the losses of a learner's updates -> {'PG_obj': mean(-pg), 'TD_loss': median(td)} like train_rl; pg: NaN where the actor did not step"""
    pg = [x for x in pg if not np.isnan(x)]
    return {'PG_obj': float(np.mean([-x for x in pg])) if len(pg) else float('nan'), 'TD_loss': float(np.median(td))}


def draw_noise(n_updates, batch, state_dim, action_dim, iteration0, policy_update_freq, caps, generator=None):
    """The draws of n_updates consecutive update_parameters calls from a torch CPU generator, in the order a CPU run of the reference
    consumes them: per update randn [B, A] (the target-policy noise, td3.py:138), and at actor updates with CAPS rand [B, S]
    (td3.py:186).  -> (target_noise f32 [n_updates, B, A], caps_noise f32 [actor updates, B, S] or None)"""
    tn, cn = [], []
    for u in range(n_updates):
        tn.append(torch.randn(batch, action_dim, generator=generator))
        if caps and (iteration0 + u + 1) % policy_update_freq == 0:
            cn.append(torch.rand(batch, state_dim, generator=generator))
    tn = torch.stack(tn) if tn else torch.zeros(0, batch, action_dim)
    if not caps:
        return tn, None
    return tn, (torch.stack(cn) if cn else torch.zeros(0, batch, state_dim))


def td3_draws(engine, *, seed, learner, iteration0, n_updates, batch, n_rows, state_dim, action_dim, policy_update_freq, caps, device=None):
    """What TD3.train(draws='device', seed=seed, learner=learner) draws in n_updates updates from iteration0 on, minibatches of `batch` of
    the first n_rows rows of a ring, written out by the kernels' own device functions (serl_td3_rng_fill)
    -> (slots i32 [n, B], target_noise f32 [n, B, A], caps_noise f32 [actor updates, B, S] or None without `caps`), device tensors: the
    tables with which serl_td3_train reproduces the call bit for bit (batch > 128: serl_td3_rng_fill_big, the tables of serl_td3_train_big)."""
    from . import _capi
    dev = torch.device(engine.device if device is None else device)
    n, B, S, A, freq, it0 = int(n_updates), int(batch), int(state_dim), int(action_dim), int(policy_update_freq), int(iteration0)
    if n < 0 or freq < 1 or it0 < 0:
        raise ValueError('td3_draws: n_updates >= 0, policy_update_freq >= 1, iteration0 >= 0')
    k = (it0 + n) // freq - it0 // freq
    slots = torch.zeros(n, B, dtype=torch.int32, device=dev)
    tn = torch.zeros(n, B, A, dtype=torch.float32, device=dev)
    cn = torch.zeros(k, B, S, dtype=torch.float32, device=dev) if caps else None
    rd = _capi.Td3RngDesc(seed=_seed64(seed, 'td3_draws'), n_rows=int(n_rows), learner0=int(learner), dense=0, caps=int(bool(caps)))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    entry = 'serl_td3_rng_fill_big' if B > FUSED_MAX_BATCH else 'serl_td3_rng_fill'
    _capi.check(getattr(_capi.lib(), entry)(engine.ctx, ctypes.byref(rd), 0, S, A, B, it0, n, freq, slots.data_ptr(), tn.data_ptr(),
                                            cn.data_ptr() if cn is not None and k else None, stream), entry)
    return slots, tn, cn


def _seed64(seed, who):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2**64:
        raise ValueError('%s: seed=%r (an integer in [0, 2^64))' % (who, seed))
    return int(seed)


class TD3:
    def __init__(self, args, engine=None):
        self.args = args
        self.engine = engine
        dev = getattr(args, 'device', 'cpu')
        S, A = args.state_dim, args.action_dim
        self.buffer = _replay.DeviceReplay(args.individual_bs, dev, engine, S, A)
        self.critical_buffer = _replay.DeviceReplay(args.individual_bs, dev, engine, S, A)
        self.actor = Actor(args, init=True)
        self.actor_target = Actor(args, init=True)
        self.actor_optim = Adam(self.actor.parameters(), lr=args.lr)
        self.critic = Critic(args)
        self.critic_target = Critic(args)
        self.critic_optim = Adam(self.critic.parameters(), lr=args.lr)
        self.gamma, self.tau = args.gamma, args.tau
        _hard_update(self.actor_target, self.actor)
        _hard_update(self.critic_target, self.critic)
        self.caps_dict = dict(CAPS) if getattr(args, 'use_caps', False) else None
        self.last_path = None                   # 'fused' / 'fused-mfma' / 'fused-rng' / 'fused-mfma-rng' / 'eager': what the most recent train() ran
                                                # (batch_size > 128 on the kernel: 'fused-big' / 'fused-mfma-big' / 'fused-big-rng' / 'fused-mfma-big-rng')
        self.last_table_bytes = None            # bytes of the slot and noise tables the most recent fused train() put on the device

    # ---- one eager update (td3.py:123-198); also the fallback of train() -------------------------------------------------------------
    def update_parameters(self, batch, iteration, champion_policy=False, *, noise=None, caps_noise=None):
        """`noise` (standard-normal [B, A]) and `caps_noise` (uniform [B, S]) replace the draws from torch's global generator."""
        a = self.args
        state, action, next_state, reward, done = batch
        dev = next(self.critic.parameters()).device
        state, action, next_state, reward, done = (x.to(dev) for x in (state, action, next_state, reward, done))
        with torch.no_grad():
            z = torch.randn_like(action) if noise is None else noise.to(action)
            z = (z * a.noise_sd).clamp(-a.noise_clip, a.noise_clip)
            next_action = torch.clamp(z + self.actor_target(next_state), -1, 1)
            q1t, q2t = self.critic_target(next_state, next_action)
            target_q = reward + (self.gamma * (torch.min(q1t, q2t) * (1 - done))).detach()
        q1, q2 = self.critic(state, action)
        td = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
        self.critic_optim.zero_grad()
        td.backward()
        nn.utils.clip_grad_norm_(self.critic.parameters(), MAX_GRAD_NORM)
        self.critic_optim.step()
        td_data = td.data.cpu().numpy()
        pgl = None
        if iteration % a.policy_update_freq == 0:
            self.actor_optim.zero_grad()
            q, _ = self.critic(state, self.actor(state))
            loss = -torch.mean(q)
            if self.caps_dict is not None:
                c = self.caps_dict
                a_now = self.actor(state)
                u = torch.rand_like(state) if caps_noise is None else caps_noise.to(state)
                a_bar = self.actor(state + u * c['eps_sd'])
                # as the reference writes them: both terms compare with the BATCH action
                loss = loss + c['lambda_t'] * F.mse_loss(action, a_now) + c['lambda_s'] * F.mse_loss(action, a_bar)
            loss.backward()
            nn.utils.clip_grad_norm_(self.actor.parameters(), MAX_GRAD_NORM)
            self.actor_optim.step()
            if not champion_policy:
                _soft_update(self.actor_target, self.actor, self.tau)
            _soft_update(self.critic_target, self.critic, self.tau)
            pgl = loss.data.cpu().numpy()
        return pgl, td_data

    # ---- a generation's updates ---------------------------------------------------------------------------------------------------------
    def _supported(self, device, work_bytes):
        """would the kernels whose workspace `work_bytes` (a function of the library) sizes run this learner's shape on `device`?"""
        from . import _capi
        a = self.args
        if torch.device(device).type != 'cuda' or self.engine is None or not torch.cuda.is_available():
            return False
        if a.activation_actor.lower() not in ACTIVATION_IDS:
            return False
        return getattr(_capi.lib(), work_bytes)(1, a.state_dim, a.action_dim, a.hidden_size, a.num_layers, int(a.batch_size)) > 0

    def fused_supported(self, device):
        """would serl_td3_train run this learner's shape on `device`?"""
        return self._supported(device, 'serl_td3_work_bytes')

    def fused_big_supported(self, device):
        """would serl_td3_train_big (minibatches of up to 512 rows, in chunks of 128) run this learner's shape on `device`?"""
        return self._supported(device, 'serl_td3_big_work_bytes')

    def fused_wide_supported(self, device):
        """would serl_td3_train_wide (minibatches of up to 512 rows, their chunks of 128 on parallel workgroups) run this learner's shape on
        `device`?"""
        return self._supported(device, 'serl_td3_wide_work_bytes')

    def train(self, replay, n_updates, *, iteration0, champion_target=False, rng=random, generator=None, fused=None, dense='valu',
              draws='host', seed=None, learner=0, chunks='serial'):
        """n_updates consecutive updates on minibatches of args.batch_size rows of `replay` (a DeviceReplay), update u with iteration
        iteration0 + u + 1 -- the loop of Agent.train_rl.  -> {'PG_obj': mean(-pg), 'TD_loss': median(td)} like train_rl.
        fused: None = the fused kernel where it runs (FUSED_DEFAULT), False = the eager loop, True = the kernel or an error.
        dense: 'valu' = serl_td3_train; 'mfma' = serl_td3_train_mfma, the same kernel with its Linear layers on the f32 matrix cores --
        bit for bit the same result (include/serl_amd.h), the kernel or an error, never the eager loop.  Anything else, or
        dense='mfma' with fused=False, is a ValueError before a draw is taken from `rng` / `generator`.
        draws: 'host' = as above.  'device' = serl_td3_train_rng: slots and noise are drawn inside the kernel as a function of (seed,
        learner, iteration) -- seed an integer in [0, 2^64), learner the key of this learner among those that share the seed -- from the
        first len(replay) rows of the ring; `rng` and `generator` are not touched and no table is allocated, so two calls of n1 and n2
        updates equal one of n1 + n2, and td3_draws(...) replays the draws.  The kernel (with `dense` phases) or an error, never the
        eager loop: an unknown `draws`, draws='device' without a seed or with fused=False is a ValueError, a shape or device the
        kernel does not run a RuntimeError, all before anything is drawn.
        batch_size 129 .. 512: fused=True, dense='mfma' and draws='device' run serl_td3_train_big (last_path 'fused-big',
        'fused-mfma-big', 'fused-big-rng', 'fused-mfma-big-rng') where fused_big_supported, else they are the RuntimeError above;
        fused=None stays the eager loop.  A refused fused=True is raised before anything is drawn too.
        chunks: 'serial' = as above.  'parallel' = serl_td3_train_wide for every batch_size in 1 .. 512: the minibatch's chunks of 128
        samples run on workgroups of their own and end bit for bit where serl_td3_train_big ends (include/serl_amd.h); with `dense` and
        `draws` as above, last_path 'fused-wide', 'fused-mfma-wide', 'fused-wide-rng' or 'fused-mfma-wide-rng'.  The kernel or an
        error, never the eager loop: an unknown `chunks`, or 'parallel' with fused=False, is a ValueError, a shape or device
        serl_td3_wide_work_bytes refuses a RuntimeError, both before anything is drawn; a hand-over of the kernel that ran out of time
        is a RuntimeError that names it, and nothing is copied back into the modules."""
        if chunks not in CHUNKS:
            raise ValueError('TD3.train: chunks=%r (one of %s)' % (chunks, ', '.join(repr(k) for k in CHUNKS)))
        wide = chunks == 'parallel'
        if wide and fused is not None and not fused:
            raise ValueError("TD3.train: chunks='parallel' selects a fused kernel, fused=False the eager loop")
        if dense not in DENSE:
            raise ValueError('TD3.train: dense=%r (one of %s)' % (dense, ', '.join(repr(k) for k in DENSE)))
        if dense != 'valu' and fused is not None and not fused:
            raise ValueError('TD3.train: dense=%r selects a fused kernel, fused=False the eager loop' % (dense,))
        if draws not in DRAWS:
            raise ValueError('TD3.train: draws=%r (one of %s)' % (draws, ', '.join(repr(k) for k in DRAWS)))
        if draws == 'device':
            if seed is None:
                raise ValueError("TD3.train: draws='device' needs seed= (an integer in [0, 2^64))")
            if fused is not None and not fused:
                raise ValueError("TD3.train: draws='device' selects a fused kernel, fused=False the eager loop")
            seed = _seed64(seed, 'TD3.train')
            if isinstance(learner, bool) or not isinstance(learner, (int, np.integer)) or not 0 <= int(learner) < 2**31 - 1:
                raise ValueError('TD3.train: learner=%r (an integer in [0, 2^31 - 1))' % (learner,))
        a = self.args
        n_updates, B = int(n_updates), int(a.batch_size)
        S, A = a.state_dim, a.action_dim
        if (replay.state_dim, replay.action_dim) != (S, A):
            raise ValueError('TD3.train: the ring holds rows of state_dim %d, action_dim %d, the learner takes %d, %d'
                             % (replay.state_dim, replay.action_dim, S, A))
        if n_updates <= 0:
            return dict(_NAN)
        if len(replay) < B:
            raise ValueError('TD3.train: %d rows in the ring, minibatches of %d' % (len(replay), B))
        can = self.fused_supported(replay.device)
        big = B > FUSED_MAX_BATCH and self.fused_big_supported(replay.device)      # (then `can` is False)
        if wide and not self.fused_wide_supported(replay.device):
            raise RuntimeError("TD3.train(chunks='parallel'): serl_td3_train_wide does not run this shape / device")
        if dense != 'valu' and not (can or big):
            raise RuntimeError('TD3.train(dense=%r): %s does not run this shape / device' % (dense, DENSE[dense][0]))
        if draws == 'device':
            if not (can or big):
                raise RuntimeError("TD3.train(draws='device'): serl_td3_train_rng does not run this shape / device")
            from . import _capi
            rd = _capi.Td3RngDesc(seed=seed, n_rows=len(replay), learner0=int(learner), dense=int(dense == 'mfma'),
                                  caps=int(self.caps_dict is not None))
            return self._train_fused(replay, n_updates, int(iteration0), not champion_target, dense=dense, big=big, wide=wide, rng_desc=rd)
        if fused and not (can or big):
            raise RuntimeError('TD3.train(fused=True): serl_td3_train does not run this shape / device')
        slots = _replay.sample_many(len(replay), B, n_updates, rng)
        tn, cn = draw_noise(n_updates, B, S, A, int(iteration0), int(a.policy_update_freq), self.caps_dict is not None, generator)
        use = (can and (dense != 'valu' or (FUSED_DEFAULT if fused is None else bool(fused)))) or (big and (dense != 'valu' or bool(fused)))
        if use or wide:
            return self._train_fused(replay, n_updates, int(iteration0), not champion_target, dense=dense, big=big, wide=wide,
                                     tables=(slots, tn, cn))
        td, pg = self._train_eager(replay, slots, tn, cn, int(iteration0), champion_target)
        self.last_path = 'eager'
        return _reduce(td, pg)

    def _train_eager(self, replay, slots, tn, cn, iteration0, champion_target):
        td, pg, k = [], [], 0
        freq = int(self.args.policy_update_freq)
        for u in range(len(slots)):
            it = iteration0 + u + 1
            rows = replay.rows[torch.as_tensor(slots[u], dtype=torch.int64, device=replay.device)]
            cz = None
            if cn is not None and it % freq == 0:
                cz, k = cn[k], k + 1
            pgl, t = self.update_parameters(replay.split(rows), it, champion_target, noise=tn[u], caps_noise=cz)
            td.append(float(t))
            if pgl is not None:
                pg.append(float(pgl))
        return td, pg

    def _train_fused(self, replay, n_updates, iteration0, update_actor_target, *, dense, big, wide=False, tables=None, rng_desc=None):
        """The K = 1 launch: n_updates updates with `dense` phases, on serl_td3_train_big when `big`, on serl_td3_train_wide when `wide`,
        drawing from `tables` (slots, tn, cn of the host) or inside the kernel with rng_desc (a _capi.Td3RngDesc; no table at all).
        -> {'PG_obj', 'TD_loss'}"""
        from . import _capi
        dev, L = replay.device, _capi.lib()
        entry, path = _names(dense, big, rng=rng_desc is not None, wide=wide)
        t = lambda x: x.contiguous().to(dev)
        rows, steps = _pack([self], dev)
        td, pg, work = _outputs(L, self.args, 1, n_updates, big, dev, wide)
        draws = {}
        if rng_desc is None:
            sl, tn, cn = tables
            sl, tn = t(torch.from_numpy(np.ascontiguousarray(sl, dtype=np.int32))), t(tn.to(torch.float32))
            cn = t(cn.to(torch.float32)) if cn is not None else None
            draws = dict(slots=sl.data_ptr(), slot_cols=sl.shape[1], target_noise=tn.data_ptr(),
                         caps_noise=None if cn is None else cn.data_ptr() if cn.numel() else work.data_ptr())
            tables = (sl, tn, cn)               # (alive until the synchronisation)
        self.last_table_bytes = sum(x.numel() * x.element_size() for x in tables or () if x is not None)
        d = _describe(self.args, n_updates, rows, steps, td, pg, work, ring=replay.rows.data_ptr(), **draws,
                      **_learner_fields(self, replay, iteration0, update_actor_target))
        args = [ctypes.byref(d)]
        if wide:
            status = torch.full((1,), -1, dtype=torch.int32, device=dev)
            args.append(ctypes.byref(_capi.Td3WideDesc(rng=ctypes.pointer(rng_desc) if rng_desc is not None else None, status=status.data_ptr(),
                                                       dense=int(dense == 'mfma'))))
        elif big:
            args.append(ctypes.byref(_capi.Td3BigDesc(rng=ctypes.pointer(rng_desc) if rng_desc is not None else None, dense=int(dense == 'mfma'))))
        elif rng_desc is not None:
            args.append(ctypes.byref(rng_desc))
        _capi.check(getattr(L, entry)(self.engine.ctx, *args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), entry)
        torch.cuda.synchronize(dev)
        if wide and int(status[0]) != 0:
            s = int(status[0])
            raise RuntimeError('TD3.train: serl_td3_train_wide gave up: %s ran out of time; the learner was not changed'
                               % _capi.TD3_WIDE_STATUS.get(s, 'status %d' % s))
        _unpack(self, rows, steps.cpu().tolist(), 0)
        self.last_path = path
        return _reduce(td[0].cpu().numpy(), pg[0].cpu().numpy())


# what the learners of a TD3Group must share: one launch has one network shape, one minibatch size and CAPS on or off for all
GROUP_SHARED = ('state_dim', 'action_dim', 'hidden_size', 'num_layers', 'activation_actor', 'batch_size')


class TD3Group:
    """K independent `TD3` learners of one network shape -- several seeds, a few hyper-parameter settings -- whose generations' updates run
    as ONE launch (serl_td3_train_group, include/serl_amd.h): one workgroup per learner, each with its own ring, fill, update count,
    iteration, seed, key and hyper-parameters.  batch_size 1 .. 512: above 128 rows the launch is serl_td3_train_group_big (chunks of 128
    samples, one after the other on the learner's workgroup), and train(chunks='parallel') is serl_td3_train_group_wide at every
    batch_size (K x ceil(batch_size / 128) workgroups, which must not outnumber the device's CUs).  Every learner ends bit for bit where
    its own `TD3.train(replay, n, iteration0=..., draws='device', seed=..., learner=key, dense=..., chunks=...)` would have put it."""

    def __init__(self, learners):
        learners = list(learners)
        if not learners:
            raise ValueError('TD3Group: no learners')
        for i, t in enumerate(learners):
            if not isinstance(t, TD3):
                raise ValueError('TD3Group: learner %d is %r, not a serl_amd.TD3' % (i, type(t).__name__))
        first = learners[0]
        for i, t in enumerate(learners[1:], 1):
            for f in GROUP_SHARED:
                x, y = getattr(first.args, f), getattr(t.args, f)
                if f == 'activation_actor':
                    x, y = str(x).lower(), str(y).lower()
                if x != y:
                    raise ValueError('TD3Group: learner %d differs from learner 0 in %s (%r, %r)' % (i, f, y, x))
            if (first.caps_dict is None) != (t.caps_dict is None):
                raise ValueError('TD3Group: learner %d differs from learner 0 in use_caps (CAPS is on for all learners of a launch or for none)' % i)
            x, y = (None if e is None else torch.device(e.device) for e in (first.engine, t.engine))
            if x != y:
                raise ValueError('TD3Group: learner %d differs from learner 0 in device (the engines are on %s and %s)' % (i, y, x))
        self.learners = learners

    def __len__(self):
        return len(self.learners)

    def _each(self, v, what):
        """a scalar for all learners, or one value per learner"""
        K = len(self.learners)
        if isinstance(v, (str, bytes)) or not hasattr(v, '__len__'):
            return [v] * K
        if len(v) != K:
            raise ValueError('TD3Group.train: %d values of %s for %d learners' % (len(v), what, K))
        return list(v)

    def train(self, replays, n_updates, *, iteration0, seed, key=None, champion_target=False, dense='valu', chunks='serial'):
        """Learner i runs n_updates[i] updates on minibatches of the first len(replays[i]) rows of its ring from iteration0[i] on, with the
        in-kernel draws of (seed[i], key[i]) -- `key` defaults to the learner's index -- and its own args / caps_dict.  n_updates,
        iteration0, seed, key and champion_target are scalars (for all) or sequences of one value per learner.
        -> a list of {'PG_obj', 'TD_loss'} like TD3.train's (NaN for a learner with no updates).  Everything is checked on the host
        before any device work (ValueError); it is the kernel or a RuntimeError, never the eager loop; one launch, one synchronisation.
        chunks: 'serial' (the default) = one workgroup per learner: serl_td3_train_group up to batch_size 128 (last_path
        'fused-group-rng' / 'fused-mfma-group-rng'), serl_td3_train_group_big for 129 .. 512 where every learner's fused_big_supported
        ('fused-big-group-rng' / 'fused-mfma-big-group-rng').  'parallel' = serl_td3_train_group_wide for every batch_size in 1 .. 512
        where fused_wide_supported and K x ceil(batch_size / 128) workgroups do not outnumber the device's CUs ('fused-wide-group-rng' /
        'fused-mfma-wide-group-rng'); bit for bit the serial result.  An unknown `chunks` is a ValueError; a shape, device or CU count
        the entry refuses is a RuntimeError that says which limit was hit; both before any device work, with no learner touched.  A
        learner whose hand-over ran out of time in the kernel is a RuntimeError that names learner and hand-over; nothing is unpacked
        into any module then."""
        from . import _capi
        who, K = 'TD3Group.train', len(self.learners)
        if dense not in DENSE:
            raise ValueError('%s: dense=%r (one of %s)' % (who, dense, ', '.join(repr(k) for k in DENSE)))
        if chunks not in CHUNKS:
            raise ValueError('%s: chunks=%r (one of %s)' % (who, chunks, ', '.join(repr(k) for k in CHUNKS)))
        replays = list(replays)
        if len(replays) != K:
            raise ValueError('%s: %d rings for %d learners' % (who, len(replays), K))
        is_int = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
        ns, its = self._each(n_updates, 'n_updates'), self._each(iteration0, 'iteration0')
        seeds, champs = self._each(seed, 'seed'), self._each(champion_target, 'champion_target')
        keys = list(range(K)) if key is None else self._each(key, 'key')
        a0 = self.learners[0].args
        S, A, B = a0.state_dim, a0.action_dim, int(a0.batch_size)
        for i, (t, r) in enumerate(zip(self.learners, replays)):
            if not is_int(ns[i]) or ns[i] < 0:
                raise ValueError('%s: learner %d: n_updates=%r (an integer >= 0)' % (who, i, ns[i]))
            if not is_int(its[i]) or its[i] < 0 or int(its[i]) + int(ns[i]) > 2**31 - 2:
                raise ValueError('%s: learner %d: iteration0=%r (an integer >= 0, iteration0 + n_updates below 2^31 - 1)' % (who, i, its[i]))
            seeds[i] = _seed64(seeds[i], '%s: learner %d' % (who, i))
            if not is_int(keys[i]) or not 0 <= int(keys[i]) < 2**31 - 1:
                raise ValueError('%s: learner %d: key=%r (an integer in [0, 2^31 - 1))' % (who, i, keys[i]))
            if (r.state_dim, r.action_dim) != (S, A):
                raise ValueError('%s: learner %d: the ring holds rows of state_dim %d, action_dim %d, the learners take %d, %d'
                                 % (who, i, r.state_dim, r.action_dim, S, A))
            if len(r) < B:
                raise ValueError('%s: learner %d: %d rows in the ring, minibatches of %d' % (who, i, len(r), B))
        ns, its, keys = [int(x) for x in ns], [int(x) for x in its], [int(x) for x in keys]
        seen = {}
        for i in range(K):
            if seen.setdefault((seeds[i], keys[i]), i) != i:
                raise ValueError('%s: learners %d and %d share (seed, key) = (%d, %d): they would draw the same minibatches and noise'
                                 % (who, seen[(seeds[i], keys[i])], i, seeds[i], keys[i]))
        dev = torch.device(replays[0].device)
        wide, big = chunks == 'parallel', chunks == 'serial' and B > FUSED_MAX_BATCH
        entry, path = _names(dense, big=big, group=True, wide=wide)
        can = 'fused_wide_supported' if wide else 'fused_big_supported' if big else 'fused_supported'
        if (any(torch.device(r.device) != dev for r in replays) or dev.type != 'cuda' or not torch.cuda.is_available() or
                any(t.engine is None for t in self.learners)):
            raise RuntimeError('%s: %s runs on one CUDA device, with learners that have an engine; the rings are on %s (there is no eager fall-back)'
                               % (who, entry, ', '.join(sorted({str(r.device) for r in replays}))))
        if not all(getattr(t, can)(dev) for t in self.learners):
            raise RuntimeError('%s: %s is not compiled for this shape: hidden a multiple of 4 in 4 .. 128, at most 4 hidden layers, state_dim '
                               '<= 16, action_dim <= 4, a known activation, batch_size <= %d (there is no eager fall-back)'
                               % (who, entry, FUSED_MAX_BATCH if can == 'fused_supported' else 512))
        if wide:
            cus, G = torch.cuda.get_device_properties(dev).multi_processor_count, (B + FUSED_MAX_BATCH - 1) // FUSED_MAX_BATCH
            if K * G > cus:
                raise RuntimeError("%s: chunks='parallel' needs %d learners x %d chunks = %d resident workgroups, the device has %d CUs "
                                   '(there is no eager fall-back)' % (who, K, G, K * G, cus))
        nmax = max(ns)
        if nmax == 0:
            return [dict(_NAN) for _ in range(K)]
        L = _capi.lib()
        rows, steps = _pack(self.learners, dev)
        table = (_capi.Td3LearnerRow * K)()
        for i, (t, r) in enumerate(zip(self.learners, replays)):
            table[i] = _capi.Td3LearnerRow(ring=r.rows.data_ptr(), seed=seeds[i], n_rows=len(r), n_updates=ns[i], key=keys[i],
                                           **_learner_fields(t, r, its[i], not champs[i]))
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        status = torch.full((K,), -1, dtype=torch.int32, device=dev)
        td, pg, work = _outputs(L, a0, K, nmax, big, dev, wide)
        d = _describe(a0, nmax, rows, steps, td, pg, work)
        gd = _capi.Td3GroupDesc(rows=table_d.data_ptr(), status=status.data_ptr(), dense=int(dense == 'mfma'),
                                caps=int(self.learners[0].caps_dict is not None))
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(getattr(L, entry)(self.learners[0].engine.ctx, ctypes.byref(d), ctypes.byref(gd), stream), entry)
        torch.cuda.synchronize(dev)
        bad = [(i, int(s)) for i, s in enumerate(status.cpu().tolist()) if s != 0]
        if bad:
            raise RuntimeError('%s: %s %s %s; no learner was changed' % (
                who, entry, 'gave up on' if any(s in _capi.TD3_ROW_TIMEOUTS for _, s in bad) else 'refused',
                ', '.join('learner %d (%s)' % (i, _capi.TD3_ROW_STATUS.get(s, 'status %d' % s)) for i, s in bad)))
        steps, td, pg = steps.cpu().tolist(), td.cpu().numpy(), pg.cpu().numpy()
        out = []
        for i, t in enumerate(self.learners):
            t.last_path = path
            if ns[i] == 0:                      # (as TD3.train: nothing of the learner is touched)
                out.append(dict(_NAN))
                continue
            _unpack(t, rows, steps, i)
            t.last_table_bytes = 0
            out.append(_reduce(td[i, :ns[i]], pg[i, :ns[i]]))
        return out
