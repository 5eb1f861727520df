"""ctypes loader of the C-ABI HIP extension (include/serl_amd.h).  Fails loudly when the library is
missing: the product has no CPU path."""
import collections, ctypes, os

_D = ctypes.POINTER(ctypes.c_double)
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int32)
VP = ctypes.c_void_p
LIB_PATH = os.environ.get('SERL_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'libserl_amd.so')

EXPORTS = ['serl_abi_version', 'serl_last_error', 'serl_param_count', 'serl_ctx_create', 'serl_ctx_destroy',
           'serl_ctx_load_build', 'serl_rollout', 'serl_rollout_multi', 'serl_dyn_open_loop', 'serl_debug_profile', 'serl_debug_mixed_placement', 'serl_last_rollout_ms', 'serl_last_rollout_info', 'serl_ga_clone', 'serl_ga_crossover',
           'serl_ga_mutate', 'serl_ga_scaled_perturb', 'serl_abi_layout', 'serl_ga_sensitivity', 'serl_ga_novelty',
           'serl_replay_scatter', 'serl_replay_scatter_rows', 'serl_env_state_dim', 'serl_env_action_dim',
           'serl_smoothness', 'serl_smoothness_work_size', 'serl_ga_distill', 'serl_host_sample_slots',
           'serl_venv_state_bytes', 'serl_venv_reset', 'serl_venv_step', 'serl_venv_step_auto', 'serl_venv_auto_layout',
           'serl_venv_rollout', 'serl_venv_rollout_layout', 'serl_venv_rollout_general',
           'serl_td3_train', 'serl_td3_train_mfma', 'serl_td3_work_bytes', 'serl_td3_param_count', 'serl_td3_layout',
           'serl_venv_noise_layout', 'serl_venv_reset_noise', 'serl_venv_step_auto_noise', 'serl_venv_rollout_noise',
           'serl_venv_rollout_general_noise', 'serl_venv_noise_fill', 'serl_venv_actor_forward', 'serl_host_philox', 'serl_host_uniform',
           'serl_venv_reset_wave', 'serl_venv_step_wave', 'serl_venv_step_auto_wave', 'serl_venv_reset_wave_noise', 'serl_venv_step_auto_wave_noise',
           'serl_venv_last_info', 'serl_venv_rollout_wave', 'serl_venv_rollout_wave_noise',
           'serl_rollout_noise', 'serl_rollout_noise_layout',
           'serl_td3_train_rng', 'serl_td3_rng_layout', 'serl_td3_rng_fill', 'serl_host_td3_slots',
           'serl_host_plan_rollout', 'serl_host_plan_dyn', 'serl_host_plan_multi',
           'serl_td3_train_group', 'serl_td3_group_layout',
           'serl_td3_train_big', 'serl_td3_big_layout', 'serl_td3_big_work_bytes', 'serl_td3_rng_fill_big',
           'serl_td3_train_wide', 'serl_td3_wide_layout', 'serl_td3_wide_work_bytes',
           'serl_td3_train_group_big', 'serl_td3_train_group_wide',
           'serl_ga_distill_general', 'serl_ga_distill_general_work_bytes',
           'serl_rollout_regrouped', 'serl_host_plan_rollout_regrouped', 'serl_last_rollout_weights',
           'serl_ga_sensitivity_general', 'serl_ga_sensitivity_general_work_bytes',
           'serl_ga_novelty_general', 'serl_shape_query']


class BuildDesc(ctypes.Structure):
    _fields_ = [('code', ctypes.c_int32), ('n_ro', ctypes.c_int32), ('ro_base', ctypes.c_uint64),
                ('ro', VP), ('t3', VP), ('x0', VP), ('dw0', VP), ('dt', ctypes.c_double)]


class RolloutDesc(ctypes.Structure):
    _fields_ = [('state_dim', ctypes.c_int32), ('action_dim', ctypes.c_int32), ('hidden', ctypes.c_int32),
                ('num_layers', ctypes.c_int32), ('activation', ctypes.c_int32), ('n_members', ctypes.c_int32),
                ('weights', VP), ('weight_stride', ctypes.c_int64),
                ('n_episodes', ctypes.c_int32), ('build_slot', ctypes.c_int32),
                ('member_of_episode', VP), ('faults', VP), ('ref', VP), ('ref_stride', ctypes.c_int64),
                ('err0', VP), ('action_noise', VP), ('noise_row', VP), ('sensor_noise', VP), ('sensor_row', VP), ('tick0', VP), ('t_max', ctypes.c_double),
                ('max_steps', ctypes.c_int32), ('lanes_per_wave', ctypes.c_int32),
                ('concurrent_episodes', ctypes.c_int32), ('kernel_hint', ctypes.c_int32),
                ('fitness', VP), ('length_steps', VP), ('length_t', VP), ('cost_steps', VP),
                ('actions', VP), ('states', VP), ('rewards', VP), ('transitions', VP),
                ('ref_spec', VP), ('ref_spec_stride', ctypes.c_int64),
                ('env_config', ctypes.c_int32), ('incremental', ctypes.c_int32)]


class FaultRow(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ('elev_gain', 'elev_clip', 'ail_clip', 'rudder_jam_on', 'rudder_jam', 'pad0', 'pad1', 'pad2')]


class RefSpec(ctypes.Structure):
    _fields_ = [('n_theta', ctypes.c_int32), ('n_phi', ctypes.c_int32), ('w_theta', ctypes.c_double), ('w_phi', ctypes.c_double),
                ('trim_deg', ctypes.c_double), ('t_theta', ctypes.c_double * 8), ('a_theta', ctypes.c_double * 8),
                ('t_phi', ctypes.c_double * 8), ('a_phi', ctypes.c_double * 8)]


class ReplayJob(ctypes.Structure):
    _fields_ = [('ring', VP), ('capacity', ctypes.c_int32), ('position', ctypes.c_int32), ('episode', ctypes.c_int32),
                ('length', ctypes.c_int32), ('cost_only', ctypes.c_int32), ('skip', ctypes.c_int32)]


class VenvDesc(ctypes.Structure):
    """serl_venv_desc (ABI v9): the step-wise vector env"""
    _fields_ = [('n_envs', ctypes.c_int32), ('build_slot', ctypes.c_int32), ('env_config', ctypes.c_int32), ('incremental', ctypes.c_int32),
                ('state_dim', ctypes.c_int32), ('action_dim', ctypes.c_int32), ('max_steps', ctypes.c_int32), ('pad0', ctypes.c_int32),
                ('t_max', ctypes.c_double), ('faults', VP), ('ref', VP), ('ref_stride', ctypes.c_int64), ('ref_spec', VP),
                ('ref_spec_stride', ctypes.c_int64), ('sensor_noise', VP), ('sensor_row', VP), ('err0', VP), ('tick0', VP), ('state', VP)]


class VenvAutoDesc(ctypes.Structure):
    """serl_venv_auto_desc: auto-reset inside the step (checked against the library by serl_venv_auto_layout, not part of serl_abi_layout)"""
    _fields_ = [('final_obs', VP), ('ep_return', VP), ('ep_length', VP), ('run_return', VP), ('run_length', VP), ('cursor', VP),
                ('ref_pool', VP), ('pool_rows', ctypes.c_int32), ('pad0', ctypes.c_int32)]


def expected_venv_auto_layout():
    """What serl_venv_auto_layout() must return for VenvAutoDesc to be right."""
    return [ctypes.sizeof(VenvAutoDesc)] + [getattr(VenvAutoDesc, n).offset for n, _ in VenvAutoDesc._fields_]


class VenvRolloutDesc(ctypes.Structure):
    """serl_venv_rollout_desc: K policy-driven steps in one launch (checked against the library by serl_venv_rollout_layout)"""
    _fields_ = ([(n, ctypes.c_int32) for n in ('state_dim', 'action_dim', 'hidden', 'num_layers', 'activation', 'n_members')] +
                [('weights', VP), ('weight_stride', ctypes.c_int64), ('member_of_env', VP), ('n_steps', ctypes.c_int32),
                 ('pad0', ctypes.c_int32), ('action_noise', VP)] +
                [(n, VP) for n in ('obs', 'actions', 'reward', 'done', 'final_obs', 'ep_return', 'ep_length', 'x', 'ref', 't', 'cost',
                                   'transitions')])


def expected_venv_rollout_layout():
    """What serl_venv_rollout_layout() must return for VenvRolloutDesc to be right."""
    return [ctypes.sizeof(VenvRolloutDesc)] + [getattr(VenvRolloutDesc, n).offset for n, _ in VenvRolloutDesc._fields_]


class VenvNoiseDesc(ctypes.Structure):
    """serl_venv_noise_desc: sensor / exploration noise drawn inside the env kernels (checked against the library by serl_venv_noise_layout)"""
    _fields_ = [('seed', ctypes.c_uint64), ('episode_count', VP), ('sensor', ctypes.c_int32), ('pad0', ctypes.c_int32),
                ('sensor_bias', ctypes.c_double * 7), ('sensor_scale', ctypes.c_double * 7), ('action', ctypes.c_int32), ('pad1', ctypes.c_int32),
                ('action_sd', ctypes.c_double), ('action_clip', ctypes.c_double)]


def expected_venv_noise_layout():
    """What serl_venv_noise_layout() must return for VenvNoiseDesc to be right."""
    return [ctypes.sizeof(VenvNoiseDesc)] + [getattr(VenvNoiseDesc, n).offset for n, _ in VenvNoiseDesc._fields_]


class RolloutNoiseDesc(ctypes.Structure):
    """serl_rollout_noise_desc: sensor / exploration noise drawn inside the population rollout kernels (checked against the library by serl_rollout_noise_layout)"""
    _fields_ = [('seed', ctypes.c_uint64), ('env', VP), ('episode', VP), ('sensor', ctypes.c_int32), ('pad0', ctypes.c_int32),
                ('sensor_bias', ctypes.c_double * 7), ('sensor_scale', ctypes.c_double * 7), ('action', ctypes.c_int32), ('pad1', ctypes.c_int32),
                ('action_sd', ctypes.c_double), ('action_clip', ctypes.c_double)]


def expected_rollout_noise_layout():
    """What serl_rollout_noise_layout() must return for RolloutNoiseDesc to be right."""
    return [ctypes.sizeof(RolloutNoiseDesc)] + [getattr(RolloutNoiseDesc, n).offset for n, _ in RolloutNoiseDesc._fields_]


class Td3Desc(ctypes.Structure):
    """serl_td3_desc: the fused TD3 learner (checked against the library by serl_td3_layout, not part of serl_abi_layout)"""
    _fields_ = ([(n, ctypes.c_int32) for n in ('state_dim', 'action_dim', 'hidden', 'num_layers', 'activation', 'n_learners', 'batch',
                                               'n_updates', 'capacity', 'slot_cols', 'policy_update_freq', 'iteration0',
                                               'update_actor_target', 'pad0')] +
                [(n, ctypes.c_float) for n in ('lr', 'gamma', 'tau', 'noise_sd', 'noise_clip', 'lambda_s', 'lambda_t', 'eps_sd',
                                               'max_grad_norm', 'pad1')] +
                [('actor', VP), ('actor_target', VP), ('actor_m', VP), ('actor_v', VP), ('actor_stride', ctypes.c_int64),
                 ('critic', VP), ('critic_target', VP), ('critic_m', VP), ('critic_v', VP), ('critic_stride', ctypes.c_int64),
                 ('adam_steps', VP), ('ring', VP), ('ring_stride', ctypes.c_int64), ('slots', VP), ('slots_stride', ctypes.c_int64),
                 ('target_noise', VP), ('noise_stride', ctypes.c_int64), ('caps_noise', VP), ('caps_stride', ctypes.c_int64),
                 ('td_loss', VP), ('pg_loss', VP), ('loss_stride', ctypes.c_int64), ('work', VP), ('work_bytes', ctypes.c_int64)])


def expected_td3_layout():
    """What serl_td3_layout() must return for Td3Desc to be right."""
    return [ctypes.sizeof(Td3Desc)] + [getattr(Td3Desc, n).offset for n, _ in Td3Desc._fields_]


class Td3RngDesc(ctypes.Structure):
    """serl_td3_rng_desc: the fused TD3 learner's in-kernel generator (checked against the library by serl_td3_rng_layout)"""
    _fields_ = [('seed', ctypes.c_uint64), ('n_rows', ctypes.c_int32), ('learner0', ctypes.c_int32), ('dense', ctypes.c_int32),
                ('caps', ctypes.c_int32)]


def expected_td3_rng_layout():
    """What serl_td3_rng_layout() must return for Td3RngDesc to be right."""
    return [ctypes.sizeof(Td3RngDesc)] + [getattr(Td3RngDesc, n).offset for n, _ in Td3RngDesc._fields_]


class Td3LearnerRow(ctypes.Structure):
    """serl_td3_learner_row: one learner of a serl_td3_train_group launch, read on the DEVICE (checked against the library by serl_td3_group_layout)"""
    _fields_ = ([('ring', VP), ('seed', ctypes.c_uint64)] +
                [(n, ctypes.c_int32) for n in ('capacity', 'n_rows', 'n_updates', 'iteration0', 'key', 'policy_update_freq',
                                               'update_actor_target', 'pad0')] +
                [(n, ctypes.c_float) for n in ('lr', 'gamma', 'tau', 'noise_sd', 'noise_clip', 'lambda_s', 'lambda_t', 'eps_sd')])


class Td3GroupDesc(ctypes.Structure):
    """serl_td3_group_desc: the rows and the status array of a serl_td3_train_group launch"""
    _fields_ = [('rows', VP), ('status', VP), ('dense', ctypes.c_int32), ('caps', ctypes.c_int32)]


def expected_td3_group_layout():
    """What serl_td3_group_layout() must return for Td3LearnerRow and Td3GroupDesc to be right."""
    return sum(([ctypes.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_] for T in (Td3LearnerRow, Td3GroupDesc)), [])


class Td3BigDesc(ctypes.Structure):
    """serl_td3_big_desc: the dense flavour and the optional generator of a serl_td3_train_big call (checked by serl_td3_big_layout)"""
    _fields_ = [('rng', ctypes.POINTER(Td3RngDesc)), ('dense', ctypes.c_int32), ('pad0', ctypes.c_int32)]


def expected_td3_big_layout():
    """What serl_td3_big_layout() must return for Td3BigDesc to be right."""
    return [ctypes.sizeof(Td3BigDesc)] + [getattr(Td3BigDesc, n).offset for n, _ in Td3BigDesc._fields_]


class Td3WideDesc(ctypes.Structure):
    """serl_td3_wide_desc: the optional generator, the status array and the dense flavour of a serl_td3_train_wide call (checked by
    serl_td3_wide_layout)"""
    _fields_ = [('rng', ctypes.POINTER(Td3RngDesc)), ('status', VP), ('dense', ctypes.c_int32), ('pad0', ctypes.c_int32)]


def expected_td3_wide_layout():
    """What serl_td3_wide_layout() must return for Td3WideDesc to be right."""
    return [ctypes.sizeof(Td3WideDesc)] + [getattr(Td3WideDesc, n).offset for n, _ in Td3WideDesc._fields_]


# enum serl_td3_wide_status: what serl_td3_train_wide leaves in status[p] -- 0, or the hand-over whose wait ran out of time
TD3_WIDE_STATUS = {0: 'ran', 1: 'hand-over A (critic partials to workgroup 0)', 2: 'hand-over B (the stepped critic to every workgroup)',
                   3: 'hand-over C (actor partials to workgroup 0)', 4: 'hand-over D (the stepped actor and the targets to every workgroup)'}


# enum serl_td3_row_status: what a workgroup of serl_td3_train_group writes to status[p]
TD3_ROW_STATUS = {0: 'ok', 1: 'ring is NULL', 2: 'n_updates < 0 or above the launch\'s', 3: 'iteration0 < 0 or iteration0 + n_updates overflows',
                  4: 'n_rows < batch or n_rows > capacity', 5: 'policy_update_freq < 1', 6: 'a hyper-parameter out of range or NaN'}
# SERL_TD3_ROW_HANDOVER_A .. _D (serl_td3_train_group_wide): the row was accepted, then a wait of the learner's hand-over ran out of time
TD3_ROW_HANDOVER0 = 16
TD3_ROW_TIMEOUTS = tuple(TD3_ROW_HANDOVER0 + s for s in sorted(TD3_WIDE_STATUS) if s)
TD3_ROW_STATUS.update({TD3_ROW_HANDOVER0 + s: what + ' ran out of time' for s, what in TD3_WIDE_STATUS.items() if s})


# serl_rollout_desc.kernel_hint (enum serl_kernel_hint)
class _Table(dict):
    """A table of the binding that is pinned entry by entry (its length, its values) where it was last extended: later entries ride beside it in
    `beside` -- t[key], key in t and t.get(key) find them, len(t) and iteration keep to the pinned entries."""

    def __init__(self, pinned, beside):
        super().__init__(pinned)
        self.beside = dict(beside)

    def __missing__(self, key):
        return self.beside[key]

    def __contains__(self, key):
        return super().__contains__(key) or key in self.beside

    def get(self, key, default=None):
        return self[key] if key in self else default


# SERL_KERNEL_LANEG / SERL_FAMILY_LANEG (include/serl_amd.h): the lane-per-episode population kernel for every actor shape
KERNEL_LANEG = 7
FAMILY_LANEG = 14
KERNEL_HINTS = _Table({None: 0, 'auto': 0, 'team': 1, 'wave': 2, 'half': 3, 'team2': 4, 'team4': 5, 'laneq': 6}, {'laneg': KERNEL_LANEG})
ABI_VERSION = 9
# serl_last_rollout_info out[0] (enum serl_kernel_family)
FAMILIES = _Table({0: None, 1: 'team', 2: 'teams', 3: 'teams2', 4: 'teamx', 5: 'team2', 6: 'team2s', 7: 'team4', 8: 'team4_mixed', 9: 'half', 10: 'wave', 11: 'wavex', 12: 'lane', 13: 'teamr'},
                  {FAMILY_LANEG: 'laneg'})


def expected_layout():
    """What serl_abi_layout() must return for these hand-written mirrors to be right."""
    return ([ctypes.sizeof(RolloutDesc)] + [getattr(RolloutDesc, n).offset for n, _ in RolloutDesc._fields_] +
            [ctypes.sizeof(BuildDesc), ctypes.sizeof(FaultRow), ctypes.sizeof(RefSpec), ctypes.sizeof(ReplayJob)] +
            [ctypes.sizeof(VenvDesc)] + [getattr(VenvDesc, n).offset for n, _ in VenvDesc._fields_])


_lib = None


class ExtensionMissing(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissing(
            'serl_amd HIP extension not built: %s is missing. Run `python -c "import __graft_entry__ as g; '
            'g.build()"` (or `python serl_amd/build.py`). There is no CPU fallback.' % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    L.serl_abi_version.restype = ctypes.c_int
    L.serl_last_error.restype = ctypes.c_char_p
    L.serl_param_count.argtypes = [ctypes.c_int] * 4
    L.serl_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(VP)]
    L.serl_ctx_destroy.argtypes = [VP]
    L.serl_ctx_load_build.argtypes = [VP, ctypes.c_int, ctypes.POINTER(BuildDesc)]
    L.serl_rollout.argtypes = [VP, ctypes.POINTER(RolloutDesc), VP]
    L.serl_rollout_multi.argtypes = [VP, ctypes.c_int32, ctypes.POINTER(RolloutDesc), VP]
    L.serl_dyn_open_loop.argtypes = [VP, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, VP, VP, ctypes.c_int32, ctypes.c_int32, VP]
    L.serl_debug_profile.argtypes = [VP, ctypes.POINTER(ctypes.c_ulonglong)]
    L.serl_debug_mixed_placement.argtypes = [VP, ctypes.POINTER(ctypes.c_int32)]
    L.serl_last_rollout_ms.argtypes = [VP, ctypes.POINTER(ctypes.c_float)]
    L.serl_last_rollout_info.argtypes = [VP, ctypes.POINTER(ctypes.c_int32)]
    L.serl_ga_clone.argtypes = [VP, VP, ctypes.c_int64, ctypes.c_int32, VP, VP, ctypes.c_int32, VP]
    L.serl_ga_crossover.argtypes = [VP, VP, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, VP, ctypes.c_int32, VP]
    L.serl_ga_mutate.argtypes = [VP, VP, ctypes.c_int64, ctypes.c_int32, VP, VP, VP, VP, ctypes.c_int32, VP]
    L.serl_ga_scaled_perturb.argtypes = [VP, VP, ctypes.c_int64, ctypes.c_int32, VP, VP, ctypes.c_int32, VP, VP, VP]
    L.serl_abi_layout.argtypes = [VP, ctypes.c_int32]
    i32 = ctypes.c_int32
    L.serl_ga_sensitivity.argtypes = [VP, VP, ctypes.c_int64, i32, i32, i32, i32, i32, VP, i32, VP, i32, VP, VP]
    L.serl_ga_sensitivity_general.argtypes = L.serl_ga_sensitivity.argtypes[:-1] + [VP, ctypes.c_int64, i32, VP]
    L.serl_ga_sensitivity_general_work_bytes.argtypes = [i32] * 6
    L.serl_ga_novelty.argtypes = [VP, VP, ctypes.c_int64, i32, i32, i32, i32, i32, VP, i32, VP, VP, i32, VP, VP]
    # (ctx, weights, stride, S, H, L, A, act, members, n, state_base, state_stride, action_base, action_stride, slots, n_rows, batch, max_batch, novelty, dense, stream)
    L.serl_ga_novelty_general.argtypes = [VP, VP, ctypes.c_int64, i32, i32, i32, i32, i32, VP, i32, VP, ctypes.c_int64, VP, ctypes.c_int64,
                                          VP, VP, VP, i32, VP, i32, VP]
    L.serl_replay_scatter.argtypes = [VP, VP, ctypes.c_int64, VP, i32, VP]
    L.serl_replay_scatter_rows.argtypes = [VP, VP, ctypes.c_int64, i32, i32, VP, i32, VP]
    L.serl_smoothness.argtypes = [VP, VP, ctypes.c_int64, VP, i32, i32, ctypes.c_double, VP, VP, VP]
    L.serl_smoothness_work_size.argtypes = [i32, i32]
    L.serl_ga_distill.argtypes = [VP, VP, ctypes.c_int64, i32, i32, i32, i32, i32, i32, VP, VP, VP, i32, VP, i32, VP, VP, ctypes.c_float, VP]
    L.serl_ga_distill_general.argtypes = L.serl_ga_distill.argtypes[:-1] + [VP, ctypes.c_int64, i32, VP]
    L.serl_ga_distill_general_work_bytes.argtypes = [i32] * 5
    L.serl_host_sample_slots.argtypes = [VP, ctypes.c_longlong, i32, i32, i32, VP, i32]
    L.serl_venv_state_bytes.argtypes = [i32]
    L.serl_venv_reset.argtypes = [VP, ctypes.POINTER(VenvDesc), VP, VP, VP]
    L.serl_venv_step.argtypes = [VP, ctypes.POINTER(VenvDesc), VP, i32, VP, VP, VP, VP, VP, VP, VP, VP]
    L.serl_venv_step_auto.argtypes = [VP, ctypes.POINTER(VenvDesc), VP, i32, VP, VP, VP, VP, VP, VP, VP, ctypes.POINTER(VenvAutoDesc), VP]
    L.serl_venv_auto_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_venv_rollout.argtypes = [VP, ctypes.POINTER(VenvDesc), ctypes.POINTER(VenvAutoDesc), ctypes.POINTER(VenvRolloutDesc), VP]
    L.serl_venv_rollout_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_venv_rollout_general.argtypes = L.serl_venv_rollout.argtypes
    L.serl_td3_train.argtypes = [VP, ctypes.POINTER(Td3Desc), VP]
    L.serl_td3_train_mfma.argtypes = L.serl_td3_train.argtypes
    NZ = ctypes.POINTER(VenvNoiseDesc)
    L.serl_venv_noise_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_venv_reset_noise.argtypes = [VP, ctypes.POINTER(VenvDesc), VP, VP, NZ, VP]
    L.serl_venv_step_auto_noise.argtypes = [VP, ctypes.POINTER(VenvDesc), VP, i32, VP, VP, VP, VP, VP, VP, VP, ctypes.POINTER(VenvAutoDesc), NZ, VP]
    L.serl_venv_rollout_noise.argtypes = [VP, ctypes.POINTER(VenvDesc), ctypes.POINTER(VenvAutoDesc), ctypes.POINTER(VenvRolloutDesc), NZ, VP]
    L.serl_venv_rollout_general_noise.argtypes = L.serl_venv_rollout_noise.argtypes
    L.serl_venv_noise_fill.argtypes = [VP, NZ, i32, i32, VP, VP, VP, i32, VP, VP]
    L.serl_venv_actor_forward.argtypes = [VP, ctypes.POINTER(VenvRolloutDesc), i32, VP, VP, VP]
    L.serl_venv_reset_wave.argtypes = L.serl_venv_reset.argtypes
    L.serl_venv_step_wave.argtypes = L.serl_venv_step.argtypes
    L.serl_venv_step_auto_wave.argtypes = L.serl_venv_step_auto.argtypes
    L.serl_venv_reset_wave_noise.argtypes = L.serl_venv_reset_noise.argtypes
    L.serl_venv_step_auto_wave_noise.argtypes = L.serl_venv_step_auto_noise.argtypes
    L.serl_venv_last_info.argtypes = [VP, VP]
    L.serl_venv_rollout_wave.argtypes = L.serl_venv_rollout_general.argtypes
    L.serl_venv_rollout_wave_noise.argtypes = L.serl_venv_rollout_general_noise.argtypes
    L.serl_rollout_noise.argtypes = [VP, ctypes.POINTER(RolloutDesc), ctypes.POINTER(RolloutNoiseDesc), VP]
    L.serl_rollout_noise_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_host_philox.argtypes = [ctypes.c_uint64] + [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint32)]
    L.serl_host_uniform.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.serl_td3_work_bytes.argtypes = [i32] * 6
    L.serl_td3_param_count.argtypes = [ctypes.c_int, ctypes.c_int]
    L.serl_td3_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_td3_rng_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_td3_train_rng.argtypes = [VP, ctypes.POINTER(Td3Desc), ctypes.POINTER(Td3RngDesc), VP]
    L.serl_td3_rng_fill.argtypes = [VP, ctypes.POINTER(Td3RngDesc)] + [i32] * 7 + [VP, VP, VP, VP]
    L.serl_host_td3_slots.argtypes = [ctypes.c_uint64, i32, i32, i32, i32, VP]
    L.serl_td3_group_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_td3_train_group.argtypes = [VP, ctypes.POINTER(Td3Desc), ctypes.POINTER(Td3GroupDesc), VP]
    L.serl_td3_big_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_td3_big_work_bytes.argtypes = [i32] * 6
    L.serl_td3_train_big.argtypes = [VP, ctypes.POINTER(Td3Desc), ctypes.POINTER(Td3BigDesc), VP]
    L.serl_td3_rng_fill_big.argtypes = L.serl_td3_rng_fill.argtypes
    L.serl_td3_wide_layout.argtypes = [VP, ctypes.c_int32]
    L.serl_td3_wide_work_bytes.argtypes = [i32] * 6
    L.serl_td3_train_wide.argtypes = [VP, ctypes.POINTER(Td3Desc), ctypes.POINTER(Td3WideDesc), VP]
    L.serl_td3_train_group_big.argtypes = L.serl_td3_train_group.argtypes
    L.serl_td3_train_group_wide.argtypes = L.serl_td3_train_group.argtypes
    L.serl_host_plan_rollout.argtypes = [_I, ctypes.POINTER(RolloutDesc), i32, _I]
    L.serl_host_plan_dyn.argtypes = [_I, i32, i32, i32, _I]
    L.serl_rollout_regrouped.argtypes = [VP, ctypes.POINTER(RolloutDesc), ctypes.POINTER(RolloutNoiseDesc), VP]
    L.serl_host_plan_rollout_regrouped.argtypes = L.serl_host_plan_rollout.argtypes
    L.serl_last_rollout_weights.argtypes = [VP, ctypes.POINTER(ctypes.c_int64)]
    L.serl_host_plan_multi.argtypes = [i32, i32, _I, i32, _I, _I, _I]
    L.serl_shape_query.argtypes = [VP, i32, i32, i32, i32, i32, i32, i32, ctypes.c_int64, _I]
    for f in EXPORTS:
        if f == 'serl_host_uniform':
            L.serl_host_uniform.restype = ctypes.c_double
        elif f == 'serl_host_philox':
            L.serl_host_philox.restype = None
        elif f not in ('serl_last_error',):
            getattr(L, f).restype = ctypes.c_longlong if f in ('serl_host_sample_slots', 'serl_venv_state_bytes', 'serl_td3_work_bytes', 'serl_td3_big_work_bytes', 'serl_td3_wide_work_bytes', 'serl_ga_distill_general_work_bytes', 'serl_ga_sensitivity_general_work_bytes') else ctypes.c_int
    if L.serl_abi_version() != ABI_VERSION:
        raise RuntimeError('serl_amd: ABI version mismatch (library %d, binding %d): rebuild with `python serl_amd/build.py`'
                           % (L.serl_abi_version(), ABI_VERSION))
    want = expected_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_abi_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: struct layout of the ctypes mirrors differs from the library (serl_abi_layout): '
                           'library %s, binding %s' % (list(got)[:n], want))
    want = expected_td3_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_td3_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the Td3Desc mirror differs from the library (serl_td3_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_td3_rng_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_td3_rng_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the Td3RngDesc mirror differs from the library (serl_td3_rng_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_td3_group_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_td3_group_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the Td3LearnerRow / Td3GroupDesc mirrors differs from the library (serl_td3_group_layout): '
                           'library %s, binding %s' % (list(got)[:n], want))
    want = expected_td3_big_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_td3_big_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the Td3BigDesc mirror differs from the library (serl_td3_big_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_td3_wide_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_td3_wide_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the Td3WideDesc mirror differs from the library (serl_td3_wide_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_venv_auto_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_venv_auto_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the VenvAutoDesc mirror differs from the library (serl_venv_auto_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_venv_rollout_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_venv_rollout_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the VenvRolloutDesc mirror differs from the library (serl_venv_rollout_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_venv_noise_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_venv_noise_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the VenvNoiseDesc mirror differs from the library (serl_venv_noise_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    want = expected_rollout_noise_layout()
    got = (ctypes.c_int32 * len(want))()
    n = L.serl_rollout_noise_layout(got, len(want))
    if n != len(want) or list(got) != want:
        raise RuntimeError('serl_amd: layout of the RolloutNoiseDesc mirror differs from the library (serl_rollout_noise_layout): library %s, binding %s'
                           % (list(got)[:n], want))
    _lib = L
    return L


E_UNSUPPORTED = -3      # enum serl_status SERL_E_UNSUPPORTED
E_INVALID = -1          # SERL_E_INVALID


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, lib().serl_last_error().decode()))


# ---- which kernel takes an actor shape: serl_shape_query, the predicates the entry points themselves refuse through (csrc/serl_shapes.h) --------
# enum serl_shape_kernel, by the entry point's name (serl_venv_rollout_wave shares serl_venv_rollout_general's contract)
SHAPE_KERNELS = {'serl_ga_sensitivity': 0, 'serl_ga_novelty': 1, 'serl_ga_distill': 2, 'serl_td3_train': 3, 'serl_td3_train_big': 4,
                 'serl_ga_sensitivity_general': 5, 'serl_ga_novelty_general': 6, 'serl_ga_distill_general': 7, 'serl_venv_rollout': 8,
                 'serl_venv_rollout_general': 9}
SHAPE_TAKES, SHAPE_RANGE, SHAPE_LDS = 0, 1, 2      # enum serl_shape_why


class Shape(collections.namedtuple('Shape', 'what rc why message')):
    """what serl_shape_query answered for the entry point `what`: its return code for the shape, why (SHAPE_*), its message"""
    takes = property(lambda self: self.why == SHAPE_TAKES)
    lds = property(lambda self: self.why == SHAPE_LDS)          # in range, too large for the LDS per workgroup

    def check(self):
        """the error the entry point itself would raise through check()"""
        if self.rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (self.what, self.rc, self.message))


def shape_query(what, spec, batch=1, ctx=None, lds_bytes=0):
    """Would the entry point `what` run `spec` actors on minibatches of `batch` rows (the env kernels: on the env `batch` = env_config +
    3 * incremental)?  With the LDS per workgroup of the context's device, or without a context of lds_bytes.  No device work."""
    why = ctypes.c_int32(0)
    rc = lib().serl_shape_query(ctx, SHAPE_KERNELS[what], spec.state_dim, spec.action_dim, spec.hidden, spec.num_layers, spec.activation_id,
                                int(batch), int(lds_bytes), ctypes.byref(why))
    return Shape(what, rc, why.value, lib().serl_last_error().decode() if rc else '')
