"""Writes tests/golden/td3_update.npz: two chains of 20 updates run by THE REFERENCE's own TD3 (base/core/td3.py) in float32 on the
CPU with fixed seeds -- the initial rows, the ring, the minibatch slots, the noise draws it consumed (captured from torch.randn_like /
torch.rand_like), the final rows of actor, critic and both targets, and the loss sequences.  Arrays only.  Needs the reference tree
(build container): python tests/golden/make_td3_golden.py"""
import os, sys, types
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference/base')
import td3_64 as T

# tag -> (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards)
CHAINS = {'a': (7, 3, 72, 3, 'tanh', 86, 2, 0, 20, 1, 1, 'small'), 'b': (2, 1, 32, 1, 'elu', 16, 3, 1, 20, 0, 0, 'big')}
ACT = {'tanh': 0, 'elu': 1, 'relu': 2}


def critic_names(k):
    return ['l1_%d.weight' % k, 'l1_%d.bias' % k, 'lnorm1_%d.gamma' % k, 'lnorm1_%d.beta' % k, 'l2_%d.weight' % k, 'l2_%d.bias' % k,
            'lnorm2_%d.gamma' % k, 'lnorm2_%d.beta' % k, 'lout_%d.weight' % k, 'lout_%d.bias' % k]


def load_critic(m, row):
    sd, off = dict(m.named_parameters()), 0
    with torch.no_grad():
        for k in (1, 2):
            for name in critic_names(k):
                p = sd[name]
                p.copy_(torch.from_numpy(row[off:off + p.numel()]).view(p.shape))
                off += p.numel()
    assert off == len(row)


def dump_critic(m):
    sd = dict(m.named_parameters())
    return torch.cat([sd[name].detach().reshape(-1) for k in (1, 2) for name in critic_names(k)]).numpy()


def run(tag, c):
    from core import td3 as R
    from serl_amd.actor import unpack_into, pack_actor
    S, A, H, L, act, B, freq, it0, n, caps, uat, rew = c
    d = T.make_case(c, seed=1000 + len(tag) + S)
    args = types.SimpleNamespace(state_dim=S, action_dim=A, hidden_size=H, num_layers=L, activation_actor=act, device='cpu', individual_bs=64,
                                 lr=T.LR, gamma=T.GAMMA, tau=T.TAU, use_caps=bool(caps), noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP,
                                 policy_update_freq=freq)
    torch.manual_seed(7)
    agent = R.TD3(args)
    unpack_into(agent.actor, torch.from_numpy(d['actor']))
    unpack_into(agent.actor_target, torch.from_numpy(d['actor_target']))
    load_critic(agent.critic, d['critic'])
    load_critic(agent.critic_target, d['critic_target'])
    tn, cn = [], []
    randn_like, rand_like = torch.randn_like, torch.rand_like

    def rec_randn(x, *a, **k):
        z = randn_like(x, *a, **k)
        tn.append(z.numpy().copy())
        return z

    def rec_rand(x, *a, **k):
        z = rand_like(x, *a, **k)
        cn.append(z.numpy().copy())
        return z
    torch.randn_like, torch.rand_like = rec_randn, rec_rand
    td, pg = [], []
    ring = torch.from_numpy(d['ring'])
    try:
        for u in range(n):
            rows = ring[torch.from_numpy(d['slots'][u].astype(np.int64))]
            batch = (rows[:, :S], rows[:, S:S + A], rows[:, S + A:2 * S + A], rows[:, 2 * S + A:2 * S + A + 1], rows[:, 2 * S + A + 1:2 * S + A + 2])
            pgl, t = agent.update_parameters(batch, it0 + u + 1, champion_policy=not uat)
            td.append(float(t))
            pg.append(float('nan') if pgl is None else float(pgl))
    finally:
        torch.randn_like, torch.rand_like = randn_like, rand_like
    for name, p in agent.critic.named_parameters():
        assert name.startswith('bnorm') == (p.grad is None), name          # the BatchNorm parameters never get a gradient
    out = {'shape': np.array([S, A, H, L, B, freq, it0, n, caps, uat, ACT[act]], np.int32), 'actor0': d['actor'], 'actor_target0': d['actor_target'],
           'critic0': d['critic'], 'critic_target0': d['critic_target'], 'ring': d['ring'], 'slots': d['slots'], 'tn': np.stack(tn).astype(np.float32),
           'cn': np.stack(cn).astype(np.float32) if cn else np.zeros((0, B, S), np.float32),
           'actor': pack_actor(agent.actor).numpy(), 'actor_target': pack_actor(agent.actor_target).numpy(), 'critic': dump_critic(agent.critic),
           'critic_target': dump_critic(agent.critic_target), 'td': np.array(td, np.float32), 'pg': np.array(pg, np.float32)}
    assert len(tn) == n and len(cn) == (int((~np.isnan(out['pg'])).sum()) if caps else 0)
    return {tag + '_' + k: v for k, v in out.items()}


if __name__ == '__main__':
    arrays = {}
    for tag, c in CHAINS.items():
        arrays.update(run(tag, c))
    path = os.path.join(ROOT, 'tests', 'golden', 'td3_update.npz')
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), 'bytes')
