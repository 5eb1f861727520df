"""Shared by tests/test_td3_hp_host.py (CPU) and tests/test_gpu_td3_hp.py (GPU): the float64 contract of tests/td3_64.py flown across the
hyper-parameters and the warm optimiser state serl_td3_train accepts -- one field away from td3_64's constants per point, the accepted
edges (tau 0 / 1, gamma 0 / 1, noise_sd 0, noise_clip 0, eps_sd 0, lambdas 0 or negative), the reference's own defaults, the norm clip active
or inactive in every step of BOTH networks, and Adam continued from step counts of 700 and 40 000 -- on three small shapes, with the bound
each point is held to.  A plain module (not a conftest): nothing here is a fixture."""
import functools
import numpy as np
import td3_64 as T

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
# the smallest of everything (no hidden layer, three samples); an odd middle one (a quarter wavefront of samples plus one); the ABI's
# largest (S, A) with one sample more than a wavefront.  policy_update_freq 2 with an even iteration0: the first update is not an actor
# update; n_updates odd (never a multiple of freq); the actor target is updated (tau shows in both target rows).
#   key: (S, A, H, L, activation, B, freq, iteration0, n_updates)
SHAPES = {'s': (2, 1, 4, 0, 'elu', 3, 2, 0, 11), 'm': (7, 3, 20, 2, 'tanh', 17, 2, 2, 11), 'l': (16, 4, 72, 3, 'relu', 65, 2, 4, 9)}

# ---- the points ---------------------------------------------------------------------------------------------------------------------
# The reference's defaults, as serl_amd.TD3 receives them: serl_amd/td3.py:173-175 (_learner_fields) passes args.lr, args.gamma, args.tau,
# args.noise_sd, args.noise_clip and the CAPS dict of serl_amd/td3.py:32 (the reference's td3.py:115-120: lambda_s 0.5, lambda_t 0.1,
# eps_sd 0.05); MAX_GRAD_NORM 10 is serl_amd/td3.py:30 (td3.py:13).  `args` is the reference's base/parameters.py: lr 0.0004335 (:47),
# gamma 0.98 (:48), noise_sd 0.2962183114680794 (:49), tau 0.005 (:54), noise_clip 0.5 (:76).  With that lr the actor, stepped five
# times in eleven updates, moves 2.2e-3 at the most (Adam's first steps are lr each) -- below td3_64.MIN_MOVED; lr is therefore raised
# by the factor 3, to 1.3005e-3: the smallest whole factor at which every shape moves both networks by more than MIN_MOVED
# (tests/test_td3_hp_host.py asserts it).
REF_LR_FACTOR = 3.0
REF_DEFAULTS = dict(lr=REF_LR_FACTOR * 0.0004335, gamma=0.98, tau=0.005, noise_sd=0.2962183114680794, noise_clip=0.5, max_norm=10.0,
                    lambda_s=0.5, lambda_t=0.1, eps_sd=0.05)
# max_norm of the two clip points, chosen on the CPU from the float64 runs' gradient norms (tests/test_td3_hp_host.py asserts the outcome):
# over the three shapes the smallest gradient norm of any critic or actor step is 0.27 (shape 'm'), so 0.05 -- five times below it -- is
# active in every step of both networks; with 'big' rewards the largest norm of any step is 1.4e3 (a critic step of shape 's'; 5.6e2 on
# 'l', 5.1e2 on 'm'), so 1e4 is active in none.
CLIP_ACTIVE, CLIP_INACTIVE = 0.05, 1e4
#   name: (the fields that differ from td3_64.DEFAULT_HP, rewards, steps0 or None = a cold start, the shapes it runs on)
POINTS = {
    'ref_defaults': (REF_DEFAULTS, 'small', None, 'sml'),
    'tau0': (dict(tau=0.0), 'small', None, 'ml'),
    'tau1': (dict(tau=1.0), 'small', None, 'sm'),
    'gamma0': (dict(gamma=0.0), 'small', None, 'sl'),
    'gamma1': (dict(gamma=1.0), 'small', None, 'ml'),
    'noise_sd0': (dict(noise_sd=0.0), 'small', None, 'sm'),
    'noise_clip0': (dict(noise_clip=0.0), 'small', None, 'ml'),
    'noise_clip5': (dict(noise_clip=5.0), 'small', None, 'sl'),           # |0.2 z| never reaches 5: plain Gaussian smoothing
    'eps_sd0': (dict(eps_sd=0.0), 'small', None, 'ml'),
    'lambdas0': (dict(lambda_s=0.0, lambda_t=0.0), 'small', None, 'sm'),
    'lambdas_apart': (dict(lambda_s=2.0, lambda_t=0.01), 'small', None, 'ml'),
    'lambda_t_negative': (dict(lambda_s=2.0, lambda_t=-0.05), 'small', None, 'sl'),
    'clip_active': (dict(max_norm=CLIP_ACTIVE), 'small', None, 'sml'),
    'clip_inactive': (dict(max_norm=CLIP_INACTIVE), 'big', None, 'sml'),
    'warm700': ({}, 'small', (700, 350), 'sl'),
    'warm40000': ({}, 'small', (40000, 20000), 'ml'),
}
CASES = [(name, sh) for name, (_, _, _, shapes) in POINTS.items() for sh in shapes]
WARM_UPDATES = 4        # the float64 run the warm moments come from: four updates (two actor steps) on another seed's ring and draws
# Seeds pinned because the case with the seed of td3_64's formula sits on a leaky-relu kink (as td3_big.SEED_OF records for one case).
# The criterion is read off the float64 run alone: a pre-activation of a leaky-relu unit (they leave LayerNorm at unit scale, median 0.8)
# whose magnitude is below KINK = 2^-23, one float32 ulp of 1 -- its sign, and with it the unit's slope, is inside float32 rounding of
# ANY summation order, and Adam's first steps turn a flipped slope into a step of the other sign (2 lr of the 4 .. 5 lr the actor moves).
#   noise_clip0-l  formula seed: 4.7e-8 in an actor layer at an actor update (1.5e-7 in the critic); the float64 run repeated from rows
#                  perturbed by one f32 rounding (6e-8 relative) already deviates by 2e-3 .. 4e-3 x moved where seeds 1 .. 3 deviate by
#                  1.4e-5 .. 1.4e-4, and float32 torch by 7.7e-3 x moved (0.48 of the bound; seeds 1 .. 5: 4e-5 .. 6.7e-4).  Seed 1: 4.9e-6.
#   tau0-l         formula seed: 8.5e-8.  Seed 1: 2.4e-6.
# Every other case of the grid stays above 4e-7 with its formula seed; tests/test_td3_hp_host.py asserts the criterion on the whole grid.
KINK = 2.0 ** -23
SEED_OF = {('noise_clip0', 'l'): 1, ('tau0', 'l'): 1}


def case_id(c):
    return '%s-%s' % c


def tuple_of(c):
    """the td3_64 case tuple of grid case c (CAPS on, the actor target updated)"""
    name, sh = c
    return SHAPES[sh] + (1, 1, POINTS[name][1])


@functools.lru_cache(maxsize=None)
def make_case(c, seed=None):
    """td3_64.make_case's dict of grid case c with 'hp' (all nine fields), 'steps0' and, on a warm start, the four moment rows under
    td3_64.MOMENTS' names: float32, from a float64 run of WARM_UPDATES updates on the case of another seed"""
    name, sh = c
    over, _, steps0, _ = POINTS[name]
    d = T.make_case(tuple_of(c), SEED_OF.get(c) if seed is None else seed)
    d['hp'] = T.hyper(over)
    d['steps0'] = (0, 0) if steps0 is None else steps0
    if steps0 is not None:
        other = T.make_case(tuple_of(c), 9000 + (0 if seed is None else seed) + len(name) + ord(sh))
        w = T.td3_literal(other, n=WARM_UPDATES)
        for k in T.MOMENTS:
            d[k] = w[k].astype(np.float32)
            assert np.abs(d[k]).max() > 0, k
    return d


def state_of(d):
    """the keyword arguments td3_64.td3_literal / td3_explicit64 take for case dict d"""
    return dict(hp=d['hp'], steps0=d['steps0'], moments0={k: d[k] for k in T.MOMENTS} if 'actor_m' in d else None)


def steps_taken(d):
    """adam_steps after the case's updates: steps0 + (critic steps, actor steps)"""
    return [d['steps0'][0] + d['n'], d['steps0'][1] + d['n_actor']]


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
# Calibrated as td3_64's were, and never against the kernel: td3_literal in float32 torch against float64 on CASES and five more seeds of
# each (seeds 1 .. 5; 210 runs).  Worst case per point over its shapes and seeds, each figure followed by its share of the bound td3_64
# sets for that activation -- rows: max |w32 - w64| / moved against TOL_REL; moments: against MOM_REL; forward: td_loss[0] and the first
# pg_loss against FWD_TOL:
#   point               rows                         moments                      forward
#   ref_defaults        1.7e-3 relu  (0.11)          1.8e-6 relu  (0.12)          1.4e-7 elu  (0.25)
#   tau0                6.0e-4 relu  (0.04)          7.7e-7 relu  (0.05)          5.5e-8 relu (0.10)
#   tau1                1.4e-4 elu   (0.02)          8.9e-7 elu   (0.01)          3.0e-8 elu  (0.05)
#   gamma0              5.7e-4 relu  (0.04)          1.3e-6 relu  (0.09)          3.5e-8 elu  (0.06)
#   gamma1              1.4e-3 relu  (0.09)          2.6e-6 relu  (0.17)          3.4e-8 relu (0.06)
#   noise_sd0           2.2e-4 tanh  (0.01)          2.7e-6 tanh  (0.02)          7.2e-8 elu  (0.13)
#   noise_clip0         7.7e-3 relu  (0.48)          2.4e-6 relu  (0.16)          3.8e-8 relu (0.07)
#   noise_clip5         2.2e-3 relu  (0.14)          2.4e-6 relu  (0.16)          8.7e-8 elu  (0.16)
#   eps_sd0             4.3e-4 relu  (0.03)          9.1e-7 relu  (0.06)          4.1e-8 relu (0.07)
#   lambdas0            1.6e-4 elu   (0.03)          3.4e-6 tanh  (0.02)          3.1e-8 elu  (0.06)
#   lambdas_apart       7.9e-4 relu  (0.05)          9.1e-7 relu  (0.06)          8.6e-8 relu (0.16)
#   lambda_t_negative   1.3e-3 relu  (0.08)          1.7e-6 elu   (0.02)          1.1e-7 relu (0.20)
#   clip_active         6.1e-4 relu  (0.04)          9.7e-7 relu  (0.06)          4.8e-8 elu  (0.09)
#   clip_inactive       7.3e-3 relu  (0.46)          7.4e-6 relu  (0.49)          1.4e-7 elu  (0.26)
#   warm700             1.6e-5 relu  (0.00)          7.7e-7 relu  (0.05)          8.6e-8 elu  (0.16)
#   warm40000           1.0e-5 relu  (0.00)          1.7e-6 relu  (0.11)          7.0e-8 relu (0.13)
# (for the two cases of SEED_OF the formula seed counts among the five more: noise_clip0's 7.7e-3 is that seed, on its kink; the pinned
# seed gives 5.4e-5.)  No point reaches half of any bound -- the largest, 0.48 and 0.46 / 0.49, are that seed and one extra seed of
# clip_inactive-l -- so every point keeps td3_64's bounds and BOUNDS introduces none.
# Had a point left them, it would stand here with 4 x its measured worst case (the margin td3_64 uses) for the quantity that left.
# moved: on the grid's own seeds every case moves the actor by >= 5.2e-3 and the critic by >= 1.2e-2 (MIN_MOVED is 4e-3); the warm
# starts move ten times as far, because moments of four updates meet bias corrections of 700 and 40 000 steps.
BOUNDS = {}


def tol_of(c, act):
    """dict(rel=, mom=, fwd=) for td3_64.check: td3_64's bounds for the activation unless BOUNDS holds the point's own"""
    own = BOUNDS.get(c[0], {})
    return dict(rel=own.get('rel', {}).get(act, T.TOL_REL[act]), mom=own.get('mom', {}).get(act, T.MOM_REL[act]), fwd=own.get('fwd', T.FWD_TOL))


# ---- the two points the other flavours are flown at (tests/test_gpu_td3_hp.py) -------------------------------------------------------
# the reference's defaults, and every exact edge at once on a warm optimiser
COMBINED_EDGE = dict(tau=1.0, gamma=0.0, noise_sd=0.0, lambda_s=2.0, lambda_t=0.01)
FLAVOUR_POINTS = {'ref_defaults': (REF_DEFAULTS, (0, 0)), 'combined_edge': (COMBINED_EDGE, (40000, 20000))}
# shape 'm' with a minibatch of 129 rows: serl_td3_train_big's second chunk holds one sample
BIG_CASE = SHAPES['m'][:5] + (129,) + SHAPES['m'][6:] + (1, 1, 'small')


@functools.lru_cache(maxsize=None)
def make_flavour_case(point, big=False):
    """shape 'm' (big: with 129 rows per minibatch on td3_big's ring) at one of FLAVOUR_POINTS, with 'hp' and 'steps0'; the moments start
    at zero (the step counts alone drive the bias corrections)"""
    import td3_big as TB
    over, steps0 = FLAVOUR_POINTS[point]
    d = TB.make_case(BIG_CASE) if big else T.make_case(tuple_of(('tau0', 'm')))
    d['hp'], d['steps0'] = T.hyper(over), steps0
    return d
