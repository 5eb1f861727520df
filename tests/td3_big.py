"""Shared by tests/test_td3_big_host.py (CPU) and tests/test_gpu_td3_big.py (GPU): cases for serl_td3_train_big -- minibatches of 129 .. 512
rows, walked by the kernel in chunks of 128 samples -- on rings of 640 rows, checked with td3_64's float64 contract and its tolerances as
they stand, and the chunked summation written out in float32 with switches for the slips a chunk loop invites.  A plain module."""
import numpy as np
import torch
from torch.nn import functional as F
import td3_64 as T
from td3_64 import td3_literal, check, case_id          # noqa: F401  (re-exported: the contract and the bound are td3_64's)

RING_ROWS = 640
CHUNK = 128
LOUD_ROWS = 160         # the ring's last rows: where the samples of a minibatch's LAST chunk come from
LOUD = 6.0              # their rewards and states are scaled by this and by 1.5: the last chunk's share of every batch sum is not a rounding error

# every B of the issue x the three shapes; rewards, CAPS, the schedule and the held actor target alternate over the grid
#   (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards)
BATCHES = (129, 192, 256, 257, 300, 512)
SHAPES = ((7, 3, 72, 3, 'tanh'), (2, 1, 4, 0, 'elu'), (16, 4, 128, 4, 'relu'))
CASES = [sh + (B, 2 if (i + j) % 3 else 3, (i + j) % 2, 13 + (i + j) % 3, int((i + j) % 4 != 3), int((i + 2 * j) % 3 != 0), 'big' if (i + j) % 2 else 'small')
         for i, B in enumerate(BATCHES) for j, sh in enumerate(SHAPES)]

# chosen on the CPU: with the seed of td3_64's formula float32 torch itself misses the bound on this case's actor (0.41 x moved: a
# leaky-relu unit on its kink; so do four of eight other seeds tried); tests/test_td3_big_host.py asserts that td3_literal in float32
# meets the bound on every case
SEED_OF = {CASES[8]: 5002}


def make_case(c, seed=None, ring_rows=RING_ROWS):
    """td3_64.make_case on a ring of ring_rows rows: the same rows, weights and draws, but the samples of the last chunk of every
    minibatch (columns from 128 * (chunks - 1) on) are drawn from the ring's LOUD_ROWS last rows, whose rewards and states are larger,
    and the others from the rows before them"""
    import actor_shapes as X
    S, A, H, L, act, B, freq, it0, n, caps, uat, rew = c
    if seed is None:
        seed = SEED_OF.get(tuple(c), S * 131 + A * 17 + H * 5 + L * 3 + B * 7 + freq + it0 + len(act))
    rng = np.random.default_rng(seed)
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)
    Pa = T.actor_param_count(S, A, H, L)
    wa = X.make_weights(s, 2, seed)[:, :Pa]
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        wc = np.stack([T._critic_row(S, A, act, gen), T._critic_row(S, A, act, gen)])
    ring = np.zeros((ring_rows, 2 * S + A + 3), np.float32)
    quiet = ring_rows - LOUD_ROWS
    scale = np.where(np.arange(ring_rows) >= quiet, 1.5, 1.0)[:, None]
    st = rng.standard_normal((ring_rows, S)) * rng.uniform(0.3, 1.5, S) * scale
    ring[:, :S] = st
    ring[:, S:S + A] = rng.uniform(-1, 1, (ring_rows, A))
    ring[:, S + A:2 * S + A] = st + 0.1 * rng.standard_normal((ring_rows, S))
    ring[:, 2 * S + A] = (-0.5 + 0.4 * rng.standard_normal(ring_rows)) * (60.0 if rew == 'big' else 0.1) * np.where(scale[:, 0] > 1.0, LOUD, 1.0)
    ring[:, 2 * S + A + 1] = rng.random(ring_rows) < 0.15
    ring[:, 2 * S + A + 2] = rng.random(ring_rows) < 0.3
    head = CHUNK * ((B - 1) // CHUNK)               # samples before the last chunk
    slots = np.stack([np.concatenate([rng.choice(quiet, head, replace=False), quiet + rng.choice(LOUD_ROWS, B - head, replace=False)])
                      for _ in range(n)]).astype(np.int32)
    n_actor = sum(1 for u in range(n) if (it0 + u + 1) % freq == 0)
    tn = rng.standard_normal((n, B, A)).astype(np.float32)
    cn = rng.random((n_actor, B, S)).astype(np.float32) if caps else None
    return dict(s=s, S=S, A=A, H=H, L=L, act=act, B=B, freq=freq, it0=it0, n=n, caps=bool(caps), uat=bool(uat), rew=rew, n_actor=n_actor,
                actor=wa[0].copy(), actor_target=wa[1].copy(), critic=wc[0], critic_target=wc[1], ring=ring, slots=slots, tn=tn, cn=cn)


# ---- the chunked summation in float32, with switches for planted slips ---------------------------------------------------------------
SLIPS = ('drop_chunk', 'divide_by_chunk', 'padding_in')


def td3_chunked32(d, slip=None):
    """The updates of td3_64.td3_literal in float32 on the packed rows, every batch sum taken chunk by chunk as serl_td3_train_big defines
    it: per chunk of 128 samples the loss terms scaled by 1 / B (1 / (B A)), gradients and losses added up in ascending chunk order, one
    clip / Adam / soft update per update.  slip: None, or
      'drop_chunk'       the last chunk's gradients are not added (its losses are)
      'divide_by_chunk'  the means divide by 128, the chunk size, instead of B
      'padding_in'       the samples from B to the end of the last chunk (zero inputs, reward 0) are not masked out of the sums"""
    assert slip is None or slip in SLIPS, slip
    S, A, H, L, B = d['S'], d['A'], d['H'], d['L'], d['B']
    f32 = torch.float32
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
        return g * (y - y.mean(-1, keepdim=True)) / (y.std(-1, keepdim=True) + 1e-6) + be

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
        W, b, g, be = take(T.HC, S + A), take(T.HC), take(T.HC), take(T.HC)
        h = act(lnorm(x @ W.T + b, g, be))
        W, b, g, be = take(T.HC, T.HC), take(T.HC), take(T.HC), take(T.HC)
        h = act(lnorm(h @ W.T + b, g, be))
        W, b = take(1, T.HC), take(1)
        return h @ W.T + b

    t32 = lambda k: torch.from_numpy(np.asarray(d[k], np.float32)).clone()
    wa, wat, wc, wct = t32('actor').requires_grad_(True), t32('actor_target'), t32('critic').requires_grad_(True), t32('critic_target')
    ring, tn = t32('ring'), t32('tn')
    cn = t32('cn') if d['caps'] else None
    st = {k: [torch.zeros_like(w), torch.zeros_like(w), 0] for k, w in (('a', wa), ('c', wc))}
    div = float(CHUNK if slip == 'divide_by_chunk' else B)
    chunks = [(b0, min(B, b0 + CHUNK)) for b0 in range(0, B, CHUNK)]

    def chunk_rows(x, b0, b1, last):
        """samples b0 .. b1 of x; with the padding let in, the last chunk is filled up to 128 samples with zeros"""
        x = x[b0:b1]
        if slip == 'padding_in' and last and b1 - b0 < CHUNK:
            x = torch.cat((x, torch.zeros(CHUNK - (b1 - b0), x.shape[1], dtype=f32)))
        return x

    def step(key, w, g):
        coef = T.MAX_NORM / (g.norm() + 1e-6)
        if bool(coef < 1.0):
            g = g * coef
        s = st[key]
        s[2] += 1
        s[0] = s[0] + (g - s[0]) * (1 - T.BETA1)
        s[1] = T.BETA2 * s[1] + (1 - T.BETA2) * g * g
        with torch.no_grad():
            w -= T.LR / (1 - T.BETA1 ** s[2]) * s[0] / (s[1].sqrt() / np.sqrt(1 - T.BETA2 ** s[2]) + T.EPS)

    td, pg, k = [], [], 0
    for u in range(d['n']):
        iteration = d['it0'] + u + 1
        rows = ring[torch.from_numpy(d['slots'][u].astype(np.int64))]
        g_sum, loss_sum = torch.zeros_like(wc), 0.0
        for ci, (b0, b1) in enumerate(chunks):
            last = ci == len(chunks) - 1
            r, z = chunk_rows(rows, b0, b1, last), chunk_rows(tn[u], b0, b1, last)
            state, action, next_state = r[:, :S], r[:, S:S + A], r[:, S + A:2 * S + A]
            reward, done = r[:, 2 * S + A:2 * S + A + 1], r[:, 2 * S + A + 1:2 * S + A + 2]
            with torch.no_grad():
                noise = (z * T.NOISE_SD).clamp(-T.NOISE_CLIP, T.NOISE_CLIP)
                x2 = torch.cat((next_state, torch.clamp(noise + actor_f(wat, next_state), -1, 1)), 1)
                target_q = reward + T.GAMMA * (torch.min(critic_f(wct, x2, 0), critic_f(wct, x2, 1)) * (1 - done))
            x = torch.cat((state, action), 1)
            loss = ((critic_f(wc, x, 0) - target_q) ** 2).sum() / div + ((critic_f(wc, x, 1) - target_q) ** 2).sum() / div
            g, = torch.autograd.grad(loss, wc)
            if not (slip == 'drop_chunk' and last and ci > 0):
                g_sum = g_sum + g
            loss_sum = loss_sum + float(loss.detach())
        step('c', wc, g_sum)
        td.append(loss_sum)
        pg.append(float('nan'))
        if iteration % d['freq'] == 0:
            g_sum, loss_sum = torch.zeros_like(wa), 0.0
            for ci, (b0, b1) in enumerate(chunks):
                last = ci == len(chunks) - 1
                r = chunk_rows(rows, b0, b1, last)
                state, action = r[:, :S], r[:, S:S + A]
                a_now = actor_f(wa, state)
                pgl = -critic_f(wc, torch.cat((state, a_now), 1), 0).sum() / div
                if d['caps']:
                    bar = actor_f(wa, state + chunk_rows(cn[k], b0, b1, last) * T.CAPS['eps_sd'])
                    pgl = pgl + T.CAPS['lambda_t'] * ((action - a_now) ** 2).sum() / (div * A) + T.CAPS['lambda_s'] * ((action - bar) ** 2).sum() / (div * A)
                g, = torch.autograd.grad(pgl, wa)
                if not (slip == 'drop_chunk' and last and ci > 0):
                    g_sum = g_sum + g
                loss_sum = loss_sum + float(pgl.detach())
            k += 1
            step('a', wa, g_sum)
            with torch.no_grad():
                if d['uat']:
                    wat = wat * (1.0 - T.TAU) + wa * T.TAU
                wct = wct * (1.0 - T.TAU) + wc * T.TAU
            pg[-1] = loss_sum
    n = lambda v: v.detach().numpy().copy()
    return dict(actor=n(wa), actor_target=n(wat), critic=n(wc), critic_target=n(wct), actor_m=n(st['a'][0]), actor_v=n(st['a'][1]),
                critic_m=n(st['c'][0]), critic_v=n(st['c'][1]), td=np.array(td), pg=np.array(pg))


def slip_applies(d, slip):
    """'padding_in' needs a partial last chunk; the other two need a second chunk (every case has one)"""
    return d['B'] % CHUNK != 0 if slip == 'padding_in' else d['B'] > CHUNK
