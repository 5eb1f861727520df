"""Shared by tests/test_td3_host.py (CPU) and tests/test_gpu_td3.py (GPU): the contract of serl_td3_train -- consecutive updates of
TD3.update_parameters (base/core/td3.py:123-198) on minibatches and noise drawn beforehand -- restated literally in float64 on the
project's own torch modules with torch.optim.Adam, the same contract written out by hand with switches for planted mistakes, a grid of
cases and the tolerance an f32 implementation must meet against the float64 run.  A plain module (not a conftest): nothing here is a
fixture."""
import types
import numpy as np
import torch
from torch.nn import functional as F

LR = 2e-3               # twice the reference's default: the actor, updated every second or third step only, still moves > MIN_MOVED
GAMMA = 0.98
TAU = 0.05
NOISE_SD, NOISE_CLIP = 0.2, 0.3          # |N(0, 1)| * 0.2 exceeds 0.3 for 13 % of the draws: the clamp matters
MAX_NORM = 10.0
CAPS = dict(lambda_s=0.5, lambda_t=0.1, eps_sd=0.05)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
HC = 64
RING_ROWS = 160
# what td3_literal / td3_explicit64 run with unless told otherwise: the constants above (tests/td3_hp.py varies them one at a time)
DEFAULT_HP = dict(lr=LR, gamma=GAMMA, tau=TAU, noise_sd=NOISE_SD, noise_clip=NOISE_CLIP, max_norm=MAX_NORM, **CAPS)


def hyper(hp=None):
    """DEFAULT_HP with the fields of `hp` (a dict of some of lr, gamma, tau, noise_sd, noise_clip, max_norm, lambda_s, lambda_t, eps_sd)"""
    assert hp is None or set(hp) <= set(DEFAULT_HP), hp
    return dict(DEFAULT_HP, **(hp or {}))

# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# A covering set: minibatches of 1, 3, 64, 65, 86, 127, 128 rows (one and two wavefronts of samples, the edges of both, the default);
# hidden 4, 32, 64, 72, 96, 128; 0, 1, 2, 3 hidden layers; (S, A) of the attitude and symmetric tasks, the full incremental one and the
# ABI's edges (1, 1), (16, 4); every activation four times; policy_update_freq 1, 2, 3 with iteration0 chosen so that the first update
# is (iteration0 + 1 a multiple of freq) and is not an actor update; n_updates never a multiple of freq > 1; CAPS on and off; the actor
# target updated and held (use_champion_target); rewards 'small' (the norm clip stays inactive in every critic step) or 'big' (x 60:
# active in every critic step) -- tests/test_td3_host.py asserts which from the float64 run.
#   (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards)
CASES = [(7, 3, 72, 3, 'tanh', 86, 2, 0, 15, 1, 1, 'small'), (7, 3, 32, 3, 'elu', 128, 2, 1, 13, 1, 0, 'big'),
         (7, 3, 96, 3, 'relu', 64, 3, 2, 14, 0, 1, 'small'), (2, 1, 4, 0, 'tanh', 3, 1, 5, 12, 1, 1, 'small'),
         (16, 3, 128, 1, 'elu', 65, 2, 0, 13, 1, 0, 'big'), (1, 1, 32, 1, 'relu', 1, 3, 0, 14, 0, 1, 'small'),
         (16, 4, 128, 3, 'tanh', 127, 2, 3, 13, 1, 1, 'small'), (16, 4, 72, 0, 'relu', 128, 1, 0, 12, 1, 0, 'big'),
         (2, 1, 96, 1, 'elu', 86, 3, 0, 16, 0, 1, 'small'), (1, 1, 4, 3, 'tanh', 64, 2, 0, 15, 1, 1, 'big'),
         (7, 3, 72, 3, 'relu', 86, 2, 7, 13, 1, 0, 'small'), (7, 3, 64, 2, 'elu', 3, 2, 0, 15, 0, 1, 'small')]


def case_id(c):
    S, A, H, L, act, B, freq, it0, n, caps, uat, rew = c
    return 'S%dA%d_H%dL%d_%s_B%d_f%d_i%d_n%d_%s_%s_%s' % (S, A, H, L, act, B, freq, it0, n, 'caps' if caps else 'nocaps',
                                                          'uat' if uat else 'champ', rew)


def net_args(S, A, H, L, act, dtype_device='cpu'):
    return types.SimpleNamespace(state_dim=S, action_dim=A, hidden_size=H, num_layers=L, activation_actor=act, device=dtype_device)


def critic_param_count(S, A):
    return 2 * (HC * (S + A) + 3 * HC + HC * HC + 3 * HC + HC + 1)


def actor_param_count(S, A, H, L):
    return H * S + H + L * (H * H + 3 * H) + A * H + A


def _critic_row(S, A, act, gen):
    from serl_amd.td3 import Critic
    from serl_amd.actor import pack_critic
    m = Critic(net_args(S, A, 4, 0, act))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith('gamma'):
                p.copy_(0.5 + 1.5 * torch.rand(p.shape, generator=gen))
            elif name.endswith('beta'):
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
            elif name.startswith(('q1.out', 'q2.out')):
                p.mul_(2.0)             # (the reference starts the output layer at 0.1 x the default: Q ~ 0; here Q matters from step 1)
    return pack_critic(m).numpy()


def make_case(c, seed=None):
    """inputs of one learner: shapes and scalars, the four initial rows (targets different from their nets), a ring of RING_ROWS rows
    (about one in seven with done = 1), slots int32 [n, B] without repetition inside a minibatch, target_noise [n, B, A], caps_noise
    [actor updates, B, S] or None"""
    import actor_shapes as X
    S, A, H, L, act, B, freq, it0, n, caps, uat, rew = c
    seed = (S * 131 + A * 17 + H * 5 + L * 3 + B * 7 + freq + it0 + len(act)) if seed is None else seed
    rng = np.random.default_rng(seed)
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)
    Pa = actor_param_count(S, A, H, L)
    wa = X.make_weights(s, 2, seed)[:, :Pa]
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        wc = np.stack([_critic_row(S, A, act, gen), _critic_row(S, A, act, gen)])
    W = 2 * S + A + 3
    ring = np.zeros((RING_ROWS, W), np.float32)
    st = rng.standard_normal((RING_ROWS, S)) * rng.uniform(0.3, 1.5, S)
    ring[:, :S] = st
    ring[:, S:S + A] = rng.uniform(-1, 1, (RING_ROWS, A))
    ring[:, S + A:2 * S + A] = st + 0.1 * rng.standard_normal((RING_ROWS, S))
    ring[:, 2 * S + A] = (-0.5 + 0.4 * rng.standard_normal(RING_ROWS)) * (60.0 if rew == 'big' else 0.1)
    ring[:, 2 * S + A + 1] = rng.random(RING_ROWS) < 0.15
    ring[:, 2 * S + A + 2] = rng.random(RING_ROWS) < 0.3
    slots = np.stack([rng.choice(RING_ROWS, B, replace=False) for _ in range(n)]).astype(np.int32)
    assert ring[slots.reshape(-1), 2 * S + A + 1].any() or B * n < 8
    n_actor = sum(1 for u in range(n) if (it0 + u + 1) % freq == 0)
    tn = rng.standard_normal((n, B, A)).astype(np.float32)
    cn = rng.random((n_actor, B, S)).astype(np.float32) if caps else None
    return dict(s=s, S=S, A=A, H=H, L=L, act=act, B=B, freq=freq, it0=it0, n=n, caps=bool(caps), uat=bool(uat), rew=rew, n_actor=n_actor,
                actor=wa[0].copy(), actor_target=wa[1].copy(), critic=wc[0], critic_target=wc[1], ring=ring, slots=slots, tn=tn, cn=cn)


ROWS = ('actor', 'actor_target', 'critic', 'critic_target')
MOMENTS = ('actor_m', 'actor_v', 'critic_m', 'critic_v')


# ---- the contract, literally ----------------------------------------------------------------------------------------------------------
def td3_literal(d, dtype=torch.float64, device='cpu', n=None, hp=None, steps0=(0, 0), moments0=None):
    """td3.py:123-198 step by step on the project's Actor / Critic modules in `dtype` with torch.optim.Adam and
    nn.utils.clip_grad_norm_, the draws replaced by the given ones.  hp: see hyper().  steps0 = (critic, actor) steps taken before and
    moments0 = {a name of MOMENTS: its packed row}: loaded into the optimisers' state dicts (an optimiser with neither starts empty).
    -> dict: the four rows, Adam's moments (float64 arrays), td [n], pg [n] (NaN where the actor was not updated), clip_c / clip_a (per
    critic / actor step: was the norm clip active)"""
    from serl_amd.actor import Actor, unpack_into, unpack_critic
    from serl_amd.td3 import Critic
    S, A = d['S'], d['A']
    n = d['n'] if n is None else n
    args = net_args(S, A, d['H'], d['L'], d['act'])
    with torch.random.fork_rng(devices=[]):
        actor, actor_t, critic, critic_t = Actor(args), Actor(args), Critic(args), Critic(args)
    for m, k in ((actor, 'actor'), (actor_t, 'actor_target')):
        m.to(dtype)
        unpack_into(m, torch.from_numpy(d[k].astype(np.float64)))
        m.to(device)
    for m, k in ((critic, 'critic'), (critic_t, 'critic_target')):
        m.to(dtype)
        unpack_critic(m, torch.from_numpy(d[k].astype(np.float64)))
        m.to(device)
    hp = hyper(hp)
    a_opt = torch.optim.Adam(actor.parameters(), lr=hp['lr'])
    c_opt = torch.optim.Adam(critic.parameters(), lr=hp['lr'])
    for opt, m, key, step in ((c_opt, critic, 'critic', steps0[0]), (a_opt, actor, 'actor', steps0[1])):
        if step or moments0 is not None:
            off = 0
            for p in m.parameters():
                row = lambda k: torch.from_numpy(np.asarray(moments0[k], np.float64)[off:off + p.numel()]).to(dtype).view(p.shape).to(device).clone()
                opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=row(key + '_m') if moments0 is not None else torch.zeros_like(p),
                                    exp_avg_sq=row(key + '_v') if moments0 is not None else torch.zeros_like(p))
                off += p.numel()
    ring = torch.from_numpy(d['ring']).to(dtype).to(device)
    tn = torch.from_numpy(d['tn']).to(dtype).to(device)
    cn = torch.from_numpy(d['cn']).to(dtype).to(device) if d['caps'] else None
    td, pg, clip_c, clip_a, k = [], [], [], [], 0
    for u in range(n):
        iteration = d['it0'] + u + 1
        rows = ring[torch.from_numpy(d['slots'][u].astype(np.int64)).to(device)]
        state, action, next_state = rows[:, :S], rows[:, S:S + A], rows[:, S + A:2 * S + A]
        reward, done = rows[:, 2 * S + A:2 * S + A + 1], rows[:, 2 * S + A + 1:2 * S + A + 2]
        with torch.no_grad():
            noise = (tn[u] * hp['noise_sd']).clamp(-hp['noise_clip'], hp['noise_clip'])
            next_action = torch.clamp(noise + actor_t(next_state), -1, 1)
            tq1, tq2 = critic_t(next_state, next_action)
            next_q = torch.min(tq1, tq2) * (1 - done)
            target_q = reward + (hp['gamma'] * next_q).detach()
        q1, q2 = critic(state, action)
        loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
        c_opt.zero_grad()
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(critic.parameters(), hp['max_norm'])
        clip_c.append(bool(hp['max_norm'] / (float(norm) + 1e-6) < 1.0))
        c_opt.step()
        td.append(float(loss.detach()))
        pg.append(float('nan'))
        if iteration % d['freq'] == 0:
            a_opt.zero_grad()
            est_q1, _ = critic(state, actor(state))
            pgl = -torch.mean(est_q1)
            if d['caps']:
                now = actor(state)
                state_bar = state + cn[k] * hp['eps_sd']
                bar = actor(state_bar)
                pgl = pgl + (hp['lambda_t'] * F.mse_loss(action, now) + hp['lambda_s'] * F.mse_loss(action, bar))
            k += 1
            pgl.backward()
            norm = torch.nn.utils.clip_grad_norm_(actor.parameters(), hp['max_norm'])
            clip_a.append(bool(hp['max_norm'] / (float(norm) + 1e-6) < 1.0))
            a_opt.step()
            with torch.no_grad():
                if d['uat']:
                    for t, p in zip(actor_t.parameters(), actor.parameters()):
                        t.copy_(t * (1.0 - hp['tau']) + p * hp['tau'])
                for t, p in zip(critic_t.parameters(), critic.parameters()):
                    t.copy_(t * (1.0 - hp['tau']) + p * hp['tau'])
            pg[-1] = float(pgl.detach())
    flat = lambda ps: torch.cat([p.detach().reshape(-1) for p in ps]).double().cpu().numpy()

    def moments(opt, m, key):
        return torch.cat([(opt.state[p][key] if p in opt.state and key in opt.state[p] else torch.zeros_like(p)).reshape(-1)
                          for p in m.parameters()]).double().cpu().numpy()
    return dict(actor=flat(actor.parameters()), actor_target=flat(actor_t.parameters()), critic=flat(critic.parameters()),
                critic_target=flat(critic_t.parameters()), actor_m=moments(a_opt, actor, 'exp_avg'), actor_v=moments(a_opt, actor, 'exp_avg_sq'),
                critic_m=moments(c_opt, critic, 'exp_avg'), critic_v=moments(c_opt, critic, 'exp_avg_sq'), td=np.array(td), pg=np.array(pg),
                clip_c=clip_c, clip_a=clip_a)


# ---- the same loop written out, with switches for planted mistakes ------------------------------------------------------------------
MISTAKES = ('clip_per_critic', 'clip_always', 'no_done', 'max_of_twins', 'noise_unclamped', 'actor_every_step', 'champion_target_updated',
            'tau_swapped', 'biased_std', 'no_bias_correction', 'no_caps', 'q2_actor_loss')
# Mistakes that only a run away from DEFAULT_HP / from a cold start can show (at the defaults each of them IS the reference, so they are
# kept apart from MISTAKES, which tests/test_td3_host.py walks on the default grid): a field replaced by today's constant
# (gamma_fixed, tau_fixed, noise_fixed = noise_sd and noise_clip, eps_sd_fixed), lambda_s and lambda_t swapped, the ACTOR's clip at
# MAX_NORM whatever hp['max_norm'] says, Adam's bias corrections counted from 0 whatever steps0 says.  tests/test_td3_hp_host.py walks them.
HP_MISTAKES = ('gamma_fixed', 'tau_fixed', 'noise_fixed', 'lambdas_swapped', 'eps_sd_fixed', 'actor_clip_fixed', 'steps_restart')


def td3_explicit64(d, mistake=None, hp=None, steps0=(0, 0), moments0=None):
    """td3_literal in float64 with the forward passes, the losses, the clip, Adam and the soft updates written out on the packed rows,
    and at most one of MISTAKES / HP_MISTAKES planted.  With mistake=None it is the reference (tests/test_td3_host.py checks that)."""
    assert mistake is None or mistake in MISTAKES + HP_MISTAKES, mistake
    hp = hyper(hp)
    gamma = GAMMA if mistake == 'gamma_fixed' else hp['gamma']
    tau = TAU if mistake == 'tau_fixed' else hp['tau']
    noise_sd, noise_clip = (NOISE_SD, NOISE_CLIP) if mistake == 'noise_fixed' else (hp['noise_sd'], hp['noise_clip'])
    lambda_s, lambda_t = (hp['lambda_t'], hp['lambda_s']) if mistake == 'lambdas_swapped' else (hp['lambda_s'], hp['lambda_t'])
    eps_sd = CAPS['eps_sd'] if mistake == 'eps_sd_fixed' else hp['eps_sd']
    S, A, H, L, B = d['S'], d['A'], d['H'], d['L'], d['B']
    corr = 0 if mistake == 'biased_std' else 1
    act = {'tanh': torch.tanh, 'elu': F.elu, 'relu': lambda v: F.leaky_relu(v, 0.01)}[d['act']]

    def taker(w):
        off = [0]

        def take(*shape):
            k = int(np.prod(shape))
            v = w[off[0]:off[0] + k].view(shape)
            off[0] += k
            return v
        return take

    def lnorm(y, g, be):
        return g * (y - y.mean(-1, keepdim=True)) / (y.std(-1, keepdim=True, correction=corr) + 1e-6) + be

    def actor_f(w, x):
        take = taker(w)
        W, b = take(H, S), take(H)
        h = act(x @ W.T + b)
        for _ in range(L):
            W, b, g, be = take(H, H), take(H), take(H), take(H)
            h = act(lnorm(h @ W.T + b, g, be))
        W, b = take(A, H), take(A)
        return torch.tanh(h @ W.T + b)

    def critic_f(w, x, twin):
        P1 = w.numel() // 2
        take = taker(w[twin * P1:(twin + 1) * P1])
        W, b, g, be = take(HC, S + A), take(HC), take(HC), take(HC)
        h = act(lnorm(x @ W.T + b, g, be))
        W, b, g, be = take(HC, HC), take(HC), take(HC), take(HC)
        h = act(lnorm(h @ W.T + b, g, be))
        W, b = take(1, HC), take(1)
        return h @ W.T + b

    f64 = lambda k: torch.from_numpy(d[k].astype(np.float64)).clone()
    wa, wat, wc, wct = f64('actor').requires_grad_(True), f64('actor_target'), f64('critic').requires_grad_(True), f64('critic_target')
    ring, tn = f64('ring'), f64('tn')
    cn = f64('cn') if d['caps'] else None
    m0 = lambda k, w: torch.zeros_like(w) if moments0 is None else torch.from_numpy(np.asarray(moments0[k], np.float64)).clone()
    st = {k: [m0(key + '_m', w), m0(key + '_v', w), 0 if mistake == 'steps_restart' else int(step)]
          for k, key, w, step in (('a', 'actor', wa, steps0[1]), ('c', 'critic', wc, steps0[0]))}

    def clip(g, parts, max_norm):
        """the joint clip over g; the planted per-critic clip treats `parts` equal pieces separately"""
        g = g.clone()
        P = g.numel() // parts
        for k in range(parts):
            seg = g[k * P:(k + 1) * P]
            coef = max_norm / (seg.norm() + 1e-6)
            active = bool(coef < 1.0)
            if active or mistake == 'clip_always':
                seg.mul_(coef)
        return g, active

    def adam(key, w, g):
        s = st[key]
        s[2] += 1
        s[0] = BETA1 * s[0] + (1 - BETA1) * g
        s[1] = BETA2 * s[1] + (1 - BETA2) * g * g
        with torch.no_grad():
            if mistake == 'no_bias_correction':
                w -= hp['lr'] * s[0] / (s[1].sqrt() + EPS)
            else:
                w -= hp['lr'] / (1 - BETA1 ** s[2]) * s[0] / (s[1].sqrt() / np.sqrt(1 - BETA2 ** s[2]) + EPS)

    td, pg, clip_c, clip_a, k = [], [], [], [], 0
    for u in range(d['n']):
        iteration = d['it0'] + u + 1
        rows = ring[torch.from_numpy(d['slots'][u].astype(np.int64))]
        state, action, next_state = rows[:, :S], rows[:, S:S + A], rows[:, S + A:2 * S + A]
        reward, done = rows[:, 2 * S + A:2 * S + A + 1], rows[:, 2 * S + A + 1:2 * S + A + 2]
        with torch.no_grad():
            noise = tn[u] * noise_sd
            if mistake != 'noise_unclamped':
                noise = noise.clamp(-noise_clip, noise_clip)
            x2 = torch.cat((next_state, torch.clamp(noise + actor_f(wat, next_state), -1, 1)), 1)
            tq1, tq2 = critic_f(wct, x2, 0), critic_f(wct, x2, 1)
            nq = torch.max(tq1, tq2) if mistake == 'max_of_twins' else torch.min(tq1, tq2)
            if mistake != 'no_done':
                nq = nq * (1 - done)
            target_q = reward + gamma * nq
        x = torch.cat((state, action), 1)
        loss = ((critic_f(wc, x, 0) - target_q) ** 2).sum() / B + ((critic_f(wc, x, 1) - target_q) ** 2).sum() / B
        g, = torch.autograd.grad(loss, wc)
        g, active = clip(g, 2 if mistake == 'clip_per_critic' else 1, hp['max_norm'])
        clip_c.append(active)
        adam('c', wc, g)
        td.append(float(loss.detach()))
        pg.append(float('nan'))
        if iteration % d['freq'] == 0 or mistake == 'actor_every_step':
            a_now = actor_f(wa, state)
            pgl = -critic_f(wc, torch.cat((state, a_now), 1), 1 if mistake == 'q2_actor_loss' else 0).sum() / B
            if d['caps']:
                if mistake != 'no_caps':
                    bar = actor_f(wa, state + cn[min(k, len(cn) - 1)] * eps_sd)
                    pgl = pgl + lambda_t * ((action - a_now) ** 2).sum() / (B * A) + lambda_s * ((action - bar) ** 2).sum() / (B * A)
            k += 1
            g, = torch.autograd.grad(pgl, wa)
            g, active = clip(g, 1, MAX_NORM if mistake == 'actor_clip_fixed' else hp['max_norm'])
            clip_a.append(active)
            adam('a', wa, g)
            t1, t2 = (tau, 1.0 - tau) if mistake == 'tau_swapped' else (1.0 - tau, tau)
            with torch.no_grad():
                if d['uat'] or mistake == 'champion_target_updated':
                    wat = wat * t1 + wa * t2
                wct = wct * t1 + wc * t2
            pg[-1] = float(pgl.detach())
    n = lambda v: v.detach().numpy().copy()
    return dict(actor=n(wa), actor_target=n(wat), critic=n(wc), critic_target=n(wct), actor_m=n(st['a'][0]), actor_v=n(st['a'][1]),
                critic_m=n(st['c'][0]), critic_v=n(st['c'][1]), td=np.array(td), pg=np.array(pg), clip_c=clip_c, clip_a=clip_a)


# ---- the tolerance ------------------------------------------------------------------------------------------------------------------
# As in tests/distill64.py: Adam divides every gradient by its own running magnitude, so the deviation of an f32 implementation from the
# float64 run is measured against how far the float64 run moved the network (moved = max |w - w0| over the actor row, resp. the critic
# row); a target row is held to the bound of its network (it is a running average of it); a moment row is measured against its own
# largest entry in the float64 run.  Calibrated on the CPU with td3_literal in float32 torch against float64 over CASES and three more
# seeds of each (48 runs; tests/test_td3_host.py asserts the grid itself) -- see the figures below the definitions.
TOL_ABS = 1e-6
MIN_MOVED = 4e-3        # every case moves actor and critic by more than this


def deviations(got, ref, d):
    """-> {row: max |got - ref| / scale}: scale = moved of the network for the four rows, max |ref| for a moment row; and the moved"""
    out, moved = {}, {}
    for net in ('actor', 'critic'):
        moved[net] = np.abs(ref[net] - d[net].astype(np.float64)).max()
    for k in ROWS:
        out[k] = np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / moved[k.split('_')[0]]
    for k in MOMENTS:
        out[k] = np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30)
    return out, moved


def first_pg(r):
    i = np.nonzero(~np.isnan(r['pg']))[0]
    return None if len(i) == 0 else int(i[0])


# Calibration (td3_literal in float32 torch against float64, CASES and five more seeds of each, 72 runs), worst max |w32 - w64| / moved:
#   tanh  8.6e-3 (actor, S16 A4 H128 L3 B127), critic 2.9e-4     elu  1.4e-3 (actor, S16 A3 H128 L1 B65), critic 1.1e-4
#   relu  4.0e-3 (critic, S16 A4 H72 L0 B128, rewards 'big'), actor 6.3e-4
# a target row deviates by less than its network in every run.  TOL_REL = 4 x the worst case of the activation.  Moments, against their
# own largest entry: worst 4.4e-5 (tanh), 2.4e-5 (elu), 3.6e-6 (relu); MOM_REL = 4 x that.  Forward only -- td_loss[0], relative to
# max(|td|, 1): worst 1.3e-7; the first pg_loss likewise: 8.7e-8 -- FWD_TOL = 4 x the worse of the two.
# The planted mistakes of tests/test_td3_host.py reach from 0.018 x moved (the clip per critic: Adam undoes most of a rescaled
# gradient) to 186 x moved (tau swapped).
TOL_REL = {'tanh': 3.5e-2, 'elu': 6e-3, 'relu': 1.6e-2}
MOM_REL = {'tanh': 1.8e-4, 'elu': 1e-4, 'relu': 1.5e-5}
FWD_TOL = 5.5e-7


def check(got, ref, d, what='', tol=None):
    """assert an f32 result (rows, moments, td, pg) against the float64 run `ref` of case dict `d`; -> the deviations.  tol: None = the
    bounds above, or dict(rel=, mom=, fwd=) of a case that has bounds of its own (tests/td3_hp.py)"""
    dev, moved = deviations(got, ref, d)
    act = d['act']
    rel, mom, fwd = (tol['rel'], tol['mom'], tol['fwd']) if tol is not None else (TOL_REL[act], MOM_REL[act], FWD_TOL)
    assert moved['actor'] > MIN_MOVED and moved['critic'] > MIN_MOVED, (what, moved)
    print('TD3_DEV %-60s %s' % (what, ' '.join('%s %.2g' % (k, v) for k, v in dev.items())))
    for k in ROWS:
        assert np.isfinite(np.asarray(got[k])).all(), (what, k)
        net = k.split('_')[0]
        assert dev[k] <= rel + TOL_ABS / moved[net], '%s: %s deviates by %.3g x moved (%.3g) > %.3g' % (what, k, dev[k], moved[net], rel)
    for k in MOMENTS:
        assert dev[k] <= mom, '%s: %s deviates by %.3g of its largest entry > %.3g' % (what, k, dev[k], mom)
    e = abs(float(got['td'][0]) - ref['td'][0]) / max(abs(ref['td'][0]), 1.0)
    assert e <= fwd, '%s: td_loss[0] %.9g against %.9g (%.3g > %.3g)' % (what, got['td'][0], ref['td'][0], e, fwd)
    i = first_pg(ref)
    if i is not None:
        e = abs(float(got['pg'][i]) - ref['pg'][i]) / max(abs(ref['pg'][i]), 1.0)
        assert e <= fwd, '%s: pg_loss[%d] %.9g against %.9g (%.3g > %.3g)' % (what, i, got['pg'][i], ref['pg'][i], e, fwd)
    return dev
