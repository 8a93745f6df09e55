"""ctypes binding of ``libcobel_hip.so`` (declared in ``include/cobel_hip.h``).

The library is the product path: there is no Python/NumPy fallback.  Importing this module on a
machine without the built library raises immediately; calling a compute entry point without a
GPU fails inside HIP and surfaces as ``CobelHipError``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (COBEL_LIB: another build of the library — kernel experiments compare variants side by side)
LIB_PATH = os.environ.get('COBEL_LIB') or os.path.join(os.path.dirname(_HERE), 'lib',
                                                     'libcobel_hip.so')

OK, E_ARG, E_RANGE, E_HIP, E_UNSUPPORTED = 0, -1, -2, -3, -4
STREAM_ENV, STREAM_POLICY, STREAM_MEMORY, STREAM_POLICY_TEST, STREAM_AGENT = 0, 1, 2, 3, 4
STREAM_PMA_MEMORY, STREAM_PMA_POLICY = 5, 6
STREAM_ADQN_MEMORY = 7
SUB_DOUBLE = 1
AGENT_Q, AGENT_DYNAQ = 0, 1
F_LEARN, F_NO_REPLAY, F_EPISODIC, F_MASK_ACTIONS, F_TEST_STREAM, F_FORCE_WAVE = 1, 2, 4, 8, 16, 32
F_FORCE_LDS_MODEL, F_NO_PREFETCH, F_SR_STREAM_ROWS, F_TAB_GENERAL, F_NO_PWG = 64, 128, 256, 512, 1024
F_PWG_GLOBAL = 2048
F_SFMA_STREAM = 4096
F_REPLAY_LANE = 8192
REPLAY_WAVE, REPLAY_LANE = 0, 1
UPDATE_ONLINE, UPDATE_PLANNING = 0, 1
TAB_KERNEL_LPI, TAB_KERNEL_WPI, TAB_KERNEL_WPI_FAST, TAB_KERNEL_WPI_INDEX, TAB_KERNEL_GENERAL = range(5)
TAB_KERNEL_PWG = 5
TAB_KERNEL_WQN = 6
MAX_BATCH = 62       # updates one wavefront takes per pass; larger batches run as several passes
MAX_ACTIONS = 32     # (action masks — one byte per state — exist up to eight)
(I_STATE, I_STEP, I_TRIAL, I_CTR_ENV, I_CTR_POLICY, I_CTR_MEMORY, I_LOG_LEN, I_FLAGS,
 I_REWARD_LO, I_REWARD_HI, I_STEPS_LO, I_STEPS_HI, I_WORDS) = range(13)


class CobelHipError(RuntimeError):
    """HIP runtime failure or unsupported configuration reported by the library."""


class ParamSet(C.Structure):
    """``cobel_param_set_t`` (512 bytes; fill with ``cobel_param_set_fill``)."""
    _fields_ = [
        ('alpha', C.c_double), ('gamma', C.c_double), ('epsilon', C.c_double),
        ('model_lr', C.c_double),
        ('alpha_f', C.c_float), ('gamma_f', C.c_float), ('model_lr_f', C.c_float),
        ('reserved_', C.c_float),
        ('eps_base', C.c_double * 5), ('eps_bonus', C.c_double * 5),
        ('eps_thr', (C.c_uint64 * 3) * 16),
    ]


class SFMAParamSet(C.Structure):
    """``cobel_sfma_param_set_t`` (592 bytes; fill with ``cobel_sfma_param_set_fill``)."""
    _fields_ = [
        ('agent', ParamSet),
        ('decay_inhibition', C.c_double), ('decay_strength', C.c_double),
        ('c_step', C.c_double), ('i_step', C.c_double), ('r_threshold', C.c_double),
        ('beta', C.c_double),
        ('reward_modulation', C.c_double), ('blend', C.c_double), ('interp_fwd', C.c_double),
        ('interp_rev', C.c_double),
    ]


# the ten doubles of a set's memory part, in the order cobel_sfma_param_set_fill takes them
SFMA_SET_MEMORY = ('decay_inhibition', 'decay_strength', 'c_step', 'i_step', 'r_threshold', 'beta',
                   'reward_modulation', 'blend', 'interp_fwd', 'interp_rev')


class DQNReplay(C.Structure):
    """``cobel_dqn_replay_t``."""
    _fields_ = [
        ('w', C.c_void_p * 3), ('b', C.c_void_p * 3),
        ('w_target', C.c_void_p * 3), ('b_target', C.c_void_p * 3),
        ('m_w', C.c_void_p * 3), ('m_b', C.c_void_p * 3),
        ('v_w', C.c_void_p * 3), ('v_b', C.c_void_p * 3),
        ('steps', C.c_void_p), ('active', C.c_void_p),
        ('states', C.c_void_p), ('next_states', C.c_void_p), ('actions', C.c_void_p),
        ('rewards', C.c_void_p), ('nonterminal', C.c_void_p),
        ('n', C.c_int32), ('n_inputs', C.c_int32), ('n_hidden1', C.c_int32),
        ('n_hidden2', C.c_int32), ('n_actions', C.c_int32), ('batch', C.c_int32),
        ('is_float64', C.c_int32), ('ddqn', C.c_int32),
        ('gamma', C.c_double), ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double),
        ('eps', C.c_double), ('weight_decay', C.c_double), ('tau', C.c_double),
        ('batch_slots', C.c_void_p), ('ring_slots', C.c_int32), ('activation', C.c_int32),
        ('obs_index', C.c_void_p), ('obs_table', C.c_void_p), ('q_out', C.c_void_p),
        ('state_index', C.c_void_p), ('next_index', C.c_void_p),
    ]


ACT_RELU, ACT_TANH = 0, 1          # cobel_dqn_replay_t.activation (COBEL_ACT_*)
ACTIVATIONS = {'relu': ACT_RELU, 'tanh': ACT_TANH}


class DQNAct(C.Structure):
    """``cobel_dqn_act_t``."""
    _fields_ = [
        ('state', C.c_void_p), ('env_ctr', C.c_void_p), ('obs_table', C.c_void_p),
        ('q', C.c_void_p), ('policy_ctr', C.c_void_p), ('policy_stream', C.c_uint32),
        ('is_float64', C.c_int32), ('epsilon', C.c_double),
        ('ring_states', C.c_void_p), ('ring_next_states', C.c_void_p),
        ('ring_actions', C.c_void_p), ('ring_rewards', C.c_void_p),
        ('ring_nonterminal', C.c_void_p), ('ring_size', C.c_void_p), ('ring_head', C.c_void_p),
        ('memory_ctr', C.c_void_p),
        ('trial', C.c_void_p), ('step', C.c_void_p), ('trial_reward', C.c_void_p),
        ('active', C.c_void_p), ('adam_steps', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('stepped', C.c_void_p), ('batch_slots', C.c_void_p),
        ('n', C.c_int32), ('n_obs', C.c_int32), ('slots', C.c_int32), ('batch', C.c_int32),
        ('steps_per_trial', C.c_int32), ('trials_target', C.c_int32), ('trial_cap', C.c_int32),
        ('mon_stripes', C.c_int32),
        ('instance_base', C.c_uint32), ('reserved_', C.c_uint32), ('seed', C.c_uint64),
        ('model_rewards', C.c_void_p), ('model_states', C.c_void_p),
        ('model_nonterminal', C.c_void_p), ('model_lr', C.c_double),
        ('n_states', C.c_int32), ('reserved2_', C.c_int32),
        ('batch_state_index', C.c_void_p), ('batch_next_index', C.c_void_p),
        ('batch_actions', C.c_void_p), ('batch_rewards', C.c_void_p),
        ('batch_nonterminal', C.c_void_p),
    ]


class MLPForward(C.Structure):
    """``cobel_mlp_forward_t``."""
    _fields_ = [
        ('w', C.c_void_p * 3), ('b', C.c_void_p * 3), ('active', C.c_void_p),
        ('in_table', C.c_void_p), ('in_index', C.c_void_p), ('in_dense', C.c_void_p),
        ('out', C.c_void_p),
        ('n', C.c_int32), ('n_inputs', C.c_int32), ('n_outputs', C.c_int32),
        ('is_float64', C.c_int32),
        ('net_div', C.c_int32), ('in_div', C.c_int32), ('act_div', C.c_int32),
        ('reserved_', C.c_int32),
    ]


class MLPFit(C.Structure):
    """``cobel_mlp_fit_t``."""
    _fields_ = [
        ('w', C.c_void_p * 3), ('b', C.c_void_p * 3),
        ('w_target', C.c_void_p * 3), ('b_target', C.c_void_p * 3),
        ('m_w', C.c_void_p * 3), ('m_b', C.c_void_p * 3),
        ('v_w', C.c_void_p * 3), ('v_b', C.c_void_p * 3),
        ('steps', C.c_void_p), ('train', C.c_void_p), ('active', C.c_void_p),
        ('in_table', C.c_void_p), ('in_index', C.c_void_p), ('in_dense', C.c_void_p),
        ('targets', C.c_void_p), ('sample_mask', C.c_void_p),
        ('ep_table', C.c_void_p), ('ep_index', C.c_void_p), ('ep_dense', C.c_void_p),
        ('ep_out', C.c_void_p),
        ('n', C.c_int32), ('n_inputs', C.c_int32), ('n_outputs', C.c_int32),
        ('is_float64', C.c_int32),
        ('in_div', C.c_int32), ('tgt_div', C.c_int32), ('act_div', C.c_int32),
        ('ep_div', C.c_int32), ('ep_rows', C.c_int32), ('debug_stage', C.c_int32),
        ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
        ('weight_decay', C.c_double), ('tau', C.c_double),
    ]


class MLPActivity(C.Structure):
    """``cobel_mlp_activity_t``."""
    _fields_ = [
        ('w', C.c_void_p * 3), ('b', C.c_void_p * 3), ('probes', C.c_void_p),
        ('units', C.c_void_p), ('out', C.c_void_p),
        ('n', C.c_int32), ('n_probes', C.c_int32), ('n_inputs', C.c_int32),
        ('n_outputs', C.c_int32), ('is_float64', C.c_int32),
        ('layer', C.c_int32), ('hidden_activation', C.c_int32), ('apply', C.c_int32),
        ('n_units', C.c_int32), ('probes_per_instance', C.c_int32),
    ]


APPLY_NONE, APPLY_RELU, APPLY_TANH = 0, 1, 2    # cobel_mlp_activity_t.apply (COBEL_APPLY_*)


class DSRTargets(C.Structure):
    """``cobel_dsr_targets_t``."""
    _fields_ = [
        ('successor', C.c_void_p), ('value', C.c_void_p), ('table', C.c_void_p),
        ('state_index', C.c_void_p), ('next_index', C.c_void_p), ('actions', C.c_void_p),
        ('nonterminal', C.c_void_p), ('targets', C.c_void_p), ('took', C.c_void_p),
        ('train', C.c_void_p),
        ('n', C.c_int32), ('n_actions', C.c_int32), ('n_outputs', C.c_int32),
        ('is_float64', C.c_int32),
        ('use_dr', C.c_int32), ('follow_up', C.c_int32), ('ignore_terminality', C.c_int32),
        ('reserved_', C.c_int32),
        ('gamma', C.c_double),
    ]


class TabRun(C.Structure):
    """``cobel_tab_run_t``."""
    _fields_ = [
        ('q', C.c_void_p), ('model', C.c_void_p), ('model_index', C.c_void_p),
        ('replay_log', C.c_void_p),
        ('inst', C.c_void_p), ('action_mask', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('resp_cnt', C.c_void_p),
        ('lat_trace', C.c_void_p), ('occupancy', C.c_void_p), ('steps_done', C.c_void_p),
        ('last_exp', C.c_void_p),
        ('n', C.c_int32), ('log_cap', C.c_int32), ('trial_cap', C.c_int32),
        ('instance_base', C.c_uint32),
        ('agent', C.c_int32), ('flags', C.c_uint32), ('trials_target', C.c_int32),
        ('steps_per_trial', C.c_int32), ('step_budget', C.c_int32), ('batch', C.c_int32),
        ('alpha', C.c_double), ('gamma', C.c_double), ('epsilon', C.c_double),
        ('model_lr', C.c_double), ('seed', C.c_uint64),
        ('param_sets', C.c_void_p), ('param_index', C.c_void_p), ('n_param_sets', C.c_int32),
        ('mon_stripes', C.c_int32), ('batches_done', C.c_void_p),
        ('scratch', C.c_void_p), ('scratch_bytes', C.c_int64),
    ]


POLICY_SOFTMAX, POLICY_EXCLUSIVE, POLICY_RANDOM = 1, 2, 3     # cobel_tab_policy_run_t.policy
POLICY_MAX_ACTIONS, POLICY_MAX_STATES = 8, 1024


class TabPolicyRun(C.Structure):
    """``cobel_tab_policy_run_t``: a ``cobel_tab_run_t`` held by value, the policy and its parameter."""
    _fields_ = [
        ('run', TabRun),
        ('policy', C.c_int32), ('reserved_', C.c_int32),
        ('policy_param', C.c_double), ('policy_params', C.c_void_p),
    ]


ROLLOUT_ELEMENT_STORES = 1       # cobel_tab_rollout_t.record_flags (COBEL_ROLLOUT_*)


class TabRollout(C.Structure):
    """``cobel_tab_rollout_t``: a ``cobel_tab_run_t`` held by value and the trajectory record."""
    _fields_ = [
        ('run', TabRun),
        ('start', C.c_void_p), ('states', C.c_void_p), ('actions', C.c_void_p),
        ('length', C.c_void_p),
        ('trials', C.c_int32), ('steps', C.c_int32), ('record_flags', C.c_uint32),
        ('reserved_', C.c_int32),
    ]


class TabExp(C.Structure):
    """``cobel_tab_exp_t`` (24 bytes)."""
    _fields_ = [
        ('state', C.c_int32), ('action', C.c_int32), ('next_state', C.c_int32),
        ('nonterminal', C.c_int32), ('reward', C.c_float), ('reserved_', C.c_int32),
    ]


def tab_scratch_bytes(n: int) -> int:
    """``COBEL_TAB_SCRATCH_BYTES(n)``."""
    return (256 + 7 * (int(n) + 8)) * 4


SFMA_MODES = ('default', 'reverse', 'forward', 'blend_forward', 'blend_reverse', 'interpolate',
              'sweeping')
(SF_RANDOM, SF_DYNAMIC, SF_START_REPLAY, SF_DETERMINISTIC, SF_RECENCY, SF_C_NORMALIZE,
 SF_D_NORMALIZE, SF_R_NORMALIZE, SF_REWARD_MOD_LOCAL, SF_REWARD_MOD, SF_STATE_MOD) = (
    1 << k for k in range(11))
(SI_CLOCK, SI_EPOCH, SI_MODE, SI_FLAGS, SI_TD_LO, SI_TD_HI, SI_CTR_AGENT, SI_RESERVED,
 SI_WORDS) = range(9)
SFMA_EVENT_BYTES = 24


class SFMARun(C.Structure):
    """``cobel_sfma_run_t``."""
    _fields_ = [
        ('q', C.c_void_p), ('model', C.c_void_p), ('strength', C.c_void_p), ('stamp', C.c_void_p),
        ('inst', C.c_void_p), ('sfma_inst', C.c_void_p), ('metric', C.c_void_p),
        ('recency_tab', C.c_void_p), ('random_cdf', C.c_void_p), ('action_mask', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('resp_cnt', C.c_void_p), ('lat_trace', C.c_void_p), ('occupancy', C.c_void_p),
        ('steps_done', C.c_void_p), ('replays_done', C.c_void_p), ('last_exp', C.c_void_p),
        ('replay_trace', C.c_void_p), ('trace_len', C.c_void_p),
        ('n', C.c_int32), ('trial_cap', C.c_int32), ('trace_cap', C.c_int32),
        ('recency_len', C.c_int32), ('instance_base', C.c_uint32),
        ('flags', C.c_uint32), ('sfma_flags', C.c_uint32),
        ('trials_target', C.c_int32), ('steps_per_trial', C.c_int32), ('step_budget', C.c_int32),
        ('batch', C.c_int32), ('nb_replays', C.c_int32), ('mon_stripes', C.c_int32),
        ('alpha', C.c_double), ('gamma', C.c_double), ('epsilon', C.c_double),
        ('model_lr', C.c_double),
        ('decay_inhibition', C.c_double), ('decay_strength', C.c_double),
        ('c_step', C.c_double), ('i_step', C.c_double), ('r_threshold', C.c_double),
        ('beta', C.c_double),
        ('reward_modulation', C.c_double), ('blend', C.c_double), ('interp_fwd', C.c_double),
        ('interp_rev', C.c_double),
        ('seed', C.c_uint64),
        ('param_sets', C.c_void_p), ('param_index', C.c_void_p), ('n_param_sets', C.c_int32),
    ]


SFM_ERROR_MOD_LOCAL, SFM_ERROR_MOD, SFM_STRIDED = 1, 2, 4


class SFMAExp(C.Structure):
    """``cobel_sfma_exp_t`` (32 bytes)."""
    _fields_ = [
        ('state', C.c_int32), ('action', C.c_int32), ('next_state', C.c_int32),
        ('nonterminal', C.c_int32), ('reward', C.c_double), ('td', C.c_double),
    ]


class SFMAMem(C.Structure):
    """``cobel_sfma_mem_t``."""
    _fields_ = [
        ('model', C.c_void_p), ('strength', C.c_void_p), ('stamp', C.c_void_p),
        ('sfma_inst', C.c_void_p), ('metric', C.c_void_p), ('recency_tab', C.c_void_p),
        ('counter', C.c_void_p),
        ('n', C.c_int32), ('n_states', C.c_int32), ('n_worlds', C.c_int32),
        ('recency_len', C.c_int32), ('instance_base', C.c_uint32),
        ('flags', C.c_uint32), ('sfma_flags', C.c_uint32), ('mem_flags', C.c_uint32),
        ('model_lr', C.c_double),
        ('decay_inhibition', C.c_double), ('decay_strength', C.c_double),
        ('c_step', C.c_double), ('i_step', C.c_double), ('r_threshold', C.c_double),
        ('beta', C.c_double),
        ('reward_modulation', C.c_double), ('blend', C.c_double), ('interp_fwd', C.c_double),
        ('interp_rev', C.c_double),
        ('seed', C.c_uint64),
        ('param_sets', C.c_void_p), ('param_index', C.c_void_p), ('n_param_sets', C.c_int32),
    ]


PMA_MAX_STATES, PMA_MAX_ACTIONS = 128, 8
PMA_WIDE_MAX_STATES = 1024
PMA_MAX_SEQ = 256
(PMA_EQUAL_NEED, PMA_EQUAL_GAIN, PMA_IGNORE_BARRIERS, PMA_ALLOW_LOOPS, PMA_GAIN_ORIGINAL,
 PMA_SHARED_POLICY, PMA_WIDE, PMA_SETS) = (1 << k for k in range(8))


PMA_Q_MEMORY, PMA_Q_AGENT = 0, 1
# the ten doubles of a cobel_pma_param_set_t: the memory's seven, then the agent's three
PMA_SET_MEMORY = ('learning_rate', 'learning_rate_q', 'learning_rate_T', 'gamma', 'gamma_q',
                  'min_gain', 'epsilon')
PMA_SET_AGENT = ('alpha', 'agent_gamma', 'agent_epsilon')


class PMAParamSet(C.Structure):
    """``cobel_pma_param_set_t`` (80 bytes; fill with ``cobel_pma_param_set_fill``)."""
    _fields_ = [(name, C.c_double) for name in PMA_SET_MEMORY + PMA_SET_AGENT]


class PMAMem(C.Structure):
    """``cobel_pma_mem_t``."""
    _fields_ = [
        ('q', C.c_void_p), ('rewards', C.c_void_p), ('states', C.c_void_p),
        ('terminals', C.c_void_p), ('T', C.c_void_p), ('SR', C.c_void_p),
        ('update_mask', C.c_void_p), ('action_mask', C.c_void_p),
        ('mem_ctr', C.c_void_p), ('pol_ctr', C.c_void_p),
        ('gamma_pow', C.c_void_p), ('gamma_q_pow', C.c_void_p),
        ('n', C.c_int32), ('n_states', C.c_int32), ('n_actions', C.c_int32),
        ('pow_len', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32), ('pol_stream', C.c_uint32),
        ('reserved_', C.c_uint32),
        ('learning_rate', C.c_double), ('learning_rate_q', C.c_double),
        ('learning_rate_T', C.c_double), ('gamma', C.c_double), ('gamma_q', C.c_double),
        ('min_gain', C.c_double), ('epsilon', C.c_double),
        ('seed', C.c_uint64),
    ]


class PMAMemSets(C.Structure):
    """``cobel_pma_mem_sets_t``: a ``cobel_pma_mem_t`` with the parameter sets behind it.  Hand
    ``byref(x.mem)`` to the entry points; they read the tail under ``PMA_SETS`` in ``mem.flags``."""
    _fields_ = [
        ('mem', PMAMem),
        ('param_sets', C.c_void_p), ('param_index', C.c_void_p), ('n_param_sets', C.c_int32),
        ('reserved_', C.c_int32),
    ]


class PMARun(C.Structure):
    """``cobel_pma_run_t``."""
    _fields_ = [
        ('inst', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('resp_cnt', C.c_void_p), ('lat_trace', C.c_void_p), ('occupancy', C.c_void_p),
        ('steps_done', C.c_void_p), ('last', C.c_void_p), ('replay_out', C.c_void_p),
        ('trial_cap', C.c_int32), ('mon_stripes', C.c_int32), ('steps_per_trial', C.c_int32),
        ('batch', C.c_int32),
        ('flags', C.c_uint32), ('reserved_', C.c_uint32),
        ('alpha', C.c_double), ('gamma_pow1', C.c_double), ('epsilon', C.c_double),
    ]


METRIC_MAX_STATES, METRIC_MAX_RANK, METRIC_MAX_WORLDS = 16383, 128, 65535


def metric_work_bytes(n_worlds: int, n_states: int, max_rank: int) -> int:
    """Bytes of the workspace ``cobel_metric_dr`` takes (include/cobel_hip.h)."""
    W, S, k = int(n_worlds), int(n_states), int(max_rank)
    head = (4 * W * (1 + k) + 15) // 16 * 16
    world = ((36 * k + 7) // 8 * 8 + 8 * (9 * k + k * k + 2 * k * S) + 15) // 16 * 16
    return head + W * world


MFEC_MAX_STATES, MFEC_MAX_ACTIONS, MFEC_MAX_CAPACITY, MFEC_MAX_K = 1024, 8, 2048, 32
MFEC_MAX_FEATURES = 65536


class MFECMem(C.Structure):
    """``cobel_mfec_mem_t``."""
    _fields_ = [
        ('rdist', C.c_void_p), ('same', C.c_void_p), ('ids', C.c_void_p), ('values', C.c_void_p),
        ('times', C.c_void_p), ('len', C.c_void_p), ('clock', C.c_void_p),
        ('n', C.c_int32), ('n_states', C.c_int32), ('n_actions', C.c_int32),
        ('capacity', C.c_int32), ('k', C.c_int32), ('reserved_', C.c_int32),
    ]


class MFECRun(C.Structure):
    """``cobel_mfec_run_t``."""
    _fields_ = [
        ('inst', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('resp_cnt', C.c_void_p), ('lat_trace', C.c_void_p), ('occupancy', C.c_void_p),
        ('steps_done', C.c_void_p), ('last_exp', C.c_void_p),
        ('ep_sa', C.c_void_p), ('ep_value', C.c_void_p),
        ('trace', C.c_void_p), ('trace_len', C.c_void_p),
        ('n', C.c_int32), ('trial_cap', C.c_int32), ('mon_stripes', C.c_int32),
        ('trace_cap', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32),
        ('trials_target', C.c_int32), ('steps_per_trial', C.c_int32), ('step_budget', C.c_int32),
        ('reserved_', C.c_int32),
        ('gamma', C.c_double), ('epsilon', C.c_double), ('seed', C.c_uint64),
    ]


RW_MAX_DIM = 64
RW_POLICY_NONE, RW_POLICY_PROPORTIONAL, RW_POLICY_THRESHOLD, RW_POLICY_SIGMOID = range(4)


class Seq(C.Structure):
    """``cobel_seq_t``."""
    _fields_ = [
        ('obs_table', C.c_void_p), ('step_obs', C.c_void_p), ('step_action', C.c_void_p),
        ('step_scalar', C.c_void_p), ('step_reward', C.c_void_p), ('trial_off', C.c_void_p),
        ('schedule_of', C.c_void_p), ('cur_trial', C.c_void_p), ('cur_step', C.c_void_p),
        ('n', C.c_int32), ('dim', C.c_int32), ('n_obs', C.c_int32), ('n_actions', C.c_int32),
        ('n_schedules', C.c_int32), ('n_trials', C.c_int32), ('n_steps', C.c_int32),
        ('overwrite', C.c_int32),
    ]


class RWRun(C.Structure):
    """``cobel_rw_run_t``."""
    _fields_ = [
        ('W', C.c_void_p), ('lr', C.c_void_p), ('pol', C.c_void_p), ('pol_ctr', C.c_void_p),
        ('instance_ids', C.c_void_p), ('mid', C.c_void_p), ('trew', C.c_void_p),
        ('trial_reward', C.c_void_p), ('trial_steps', C.c_void_p), ('trial_action', C.c_void_p),
        ('trace', C.c_void_p), ('trace_len', C.c_void_p), ('steps_done', C.c_void_p),
        ('n', C.c_int32), ('trial_cap', C.c_int32), ('trace_cap', C.c_int32),
        ('lr_rows', C.c_int32), ('pol_rows', C.c_int32), ('policy', C.c_int32),
        ('code_reverse', C.c_int32), ('reserved_', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32),
        ('pol_stream', C.c_uint32), ('reserved2_', C.c_uint32),
        ('trial_first', C.c_int32), ('trials', C.c_int32), ('steps_per_trial', C.c_int32),
        ('step_budget', C.c_int32),
        ('seed', C.c_uint64),
    ]


QSEQ_MAX_ACTIONS, QSEQ_MAX_KEYS, QSEQ_ROW = 8, 64, 6
QSEQ_POLICY_SOFTMAX, QSEQ_POLICY_EPS_GREEDY = 0, 1


class QSeqRun(C.Structure):
    """``cobel_qseq_run_t``."""
    _fields_ = [
        ('Q', C.c_void_p), ('key_of_row', C.c_void_p), ('par', C.c_void_p), ('pol_ctr', C.c_void_p),
        ('mem_ctr', C.c_void_p), ('log', C.c_void_p), ('log_len', C.c_void_p),
        ('instance_ids', C.c_void_p), ('mid', C.c_void_p), ('trew', C.c_void_p),
        ('trial_reward', C.c_void_p), ('trial_steps', C.c_void_p), ('trial_action', C.c_void_p),
        ('trace', C.c_void_p), ('trace_len', C.c_void_p), ('last', C.c_void_p),
        ('steps_done', C.c_void_p),
        ('n', C.c_int32), ('n_keys', C.c_int32), ('n_actions', C.c_int32), ('log_cap', C.c_int32),
        ('trial_cap', C.c_int32), ('trace_cap', C.c_int32), ('par_rows', C.c_int32),
        ('policy', C.c_int32), ('batch_size', C.c_int32), ('reserved_', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32),
        ('pol_stream', C.c_uint32), ('reserved2_', C.c_uint32),
        ('trial_first', C.c_int32), ('trials', C.c_int32), ('steps_per_trial', C.c_int32),
        ('step_budget', C.c_int32),
        ('seed', C.c_uint64),
    ]


ANET_MAX_ACTIONS = 9


class ANetRun(C.Structure):
    """``cobel_anet_run_t``."""
    _fields_ = [
        ('We', C.c_void_p), ('Wi', C.c_void_p), ('sat_e', C.c_void_p), ('sat_i', C.c_void_p),
        ('lr_e', C.c_void_p), ('lr_i', C.c_void_p), ('eps', C.c_void_p), ('pol_ctr', C.c_void_p),
        ('agent_ctr', C.c_void_p), ('instance_ids', C.c_void_p), ('mid', C.c_void_p),
        ('trew', C.c_void_p), ('trial_reward', C.c_void_p), ('trial_steps', C.c_void_p),
        ('trial_action', C.c_void_p), ('trace', C.c_void_p), ('trace_len', C.c_void_p),
        ('steps_done', C.c_void_p),
        ('n', C.c_int32), ('n_actions', C.c_int32), ('trial_cap', C.c_int32),
        ('trace_cap', C.c_int32), ('sat_rows', C.c_int32), ('lr_rows', C.c_int32),
        ('eps_rows', C.c_int32), ('linear_update', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32),
        ('pol_stream', C.c_uint32), ('reserved_', C.c_uint32),
        ('trial_first', C.c_int32), ('trials', C.c_int32), ('steps_per_trial', C.c_int32),
        ('step_budget', C.c_int32),
        ('alpha', C.c_double), ('noise', C.c_double), ('seed', C.c_uint64),
    ]


ADQN_RPE = 1


class ADQNMem(C.Structure):
    """``cobel_adqn_mem_t``."""
    _fields_ = [
        ('states', C.c_void_p), ('reinforcements', C.c_void_p), ('errors', C.c_void_p),
        ('priorities', C.c_void_p), ('count', C.c_void_p), ('draw_ctr', C.c_void_p),
        ('instance_ids', C.c_void_p), ('scratch', C.c_void_p),
        ('n', C.c_int32), ('dim', C.c_int32), ('cap', C.c_int32),
        ('count_min', C.c_int32), ('count_max', C.c_int32),
        ('instance_base', C.c_uint32), ('flags', C.c_uint32), ('reserved_', C.c_uint32),
        ('decay', C.c_double), ('seed', C.c_uint64),
    ]


class ADQNStep(C.Structure):
    """``cobel_adqn_step_t``."""
    _fields_ = [
        ('value', C.c_void_p), ('in_index', C.c_void_p), ('targets', C.c_void_p),
        ('idx', C.c_void_p), ('ep_index', C.c_void_p), ('active', C.c_void_p),
        ('alive', C.c_void_p), ('done', C.c_void_p), ('mid', C.c_void_p), ('trew', C.c_void_p),
        ('trial_reward', C.c_void_p), ('trial_steps', C.c_void_p), ('step_rec', C.c_void_p),
        ('trace', C.c_void_p), ('idx_trace', C.c_void_p), ('trace_len', C.c_void_p),
        ('steps_done', C.c_void_p),
        ('n', C.c_int32), ('batch', C.c_int32), ('is_float64', C.c_int32),
        ('trial_cap', C.c_int32), ('trace_cap', C.c_int32), ('flags', C.c_uint32),
        ('trial_first', C.c_int32), ('trials', C.c_int32), ('steps_per_trial', C.c_int32),
        ('reserved_', C.c_int32),
    ]


C2D_MAX_EDGES, C2D_MAX_REWARDS = 1024, 32
C2D_STEP, C2D_WHEEL = 0, 1


class C2D(C.Structure):
    """``cobel_c2d_t``."""
    _fields_ = [
        ('edges', C.c_void_p), ('spawn_edges', C.c_void_p), ('rewards', C.c_void_p),
        ('state', C.c_void_p), ('env_ctr', C.c_void_p),
        ('box', C.c_double * 4), ('fallback', C.c_double * 2),
        ('step_size', C.c_double), ('body_radius', C.c_double), ('wheel_distance', C.c_double),
        ('buffer', C.c_double), ('seed', C.c_uint64),
        ('n', C.c_int32), ('n_edges', C.c_int32), ('n_spawn_edges', C.c_int32),
        ('n_rewards', C.c_int32), ('robot_type', C.c_int32), ('punish_wall', C.c_int32),
        ('lanes_per_instance', C.c_int32), ('instance_base', C.c_uint32),
    ]


class DQNActC2D(C.Structure):
    """``cobel_dqn_c2d_act_t``: ``cobel_dqn_act_t``'s policy, ring, bookkeeping and output fields
    under the same names around a ``cobel_c2d_t`` held by value."""
    _fields_ = [
        ('arena', C2D),
        ('q', C.c_void_p), ('policy_ctr', C.c_void_p), ('policy_stream', C.c_uint32),
        ('is_float64', C.c_int32), ('epsilon', C.c_double),
        ('ring_states', C.c_void_p), ('ring_next_states', C.c_void_p),
        ('ring_actions', C.c_void_p), ('ring_rewards', C.c_void_p),
        ('ring_nonterminal', C.c_void_p), ('ring_size', C.c_void_p), ('ring_head', C.c_void_p),
        ('memory_ctr', C.c_void_p),
        ('trial', C.c_void_p), ('step', C.c_void_p), ('trial_reward', C.c_void_p),
        ('active', C.c_void_p), ('adam_steps', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('stepped', C.c_void_p), ('batch_slots', C.c_void_p),
        ('obs', C.c_void_p), ('reward_out', C.c_void_p), ('done_out', C.c_void_p),
        ('wall_out', C.c_void_p), ('fallbacks', C.c_void_p),
        ('slots', C.c_int32), ('batch', C.c_int32),
        ('steps_per_trial', C.c_int32), ('trials_target', C.c_int32), ('trial_cap', C.c_int32),
        ('mon_stripes', C.c_int32),
    ]


class SRRun(C.Structure):
    """``cobel_sr_run_t``."""
    _fields_ = [
        ('sr', C.c_void_p), ('trans', C.c_void_p), ('rewards', C.c_void_p), ('inst', C.c_void_p),
        ('action_mask', C.c_void_p),
        ('lat_sum', C.c_void_p), ('lat_cnt', C.c_void_p), ('reward_sum', C.c_void_p),
        ('resp_cnt', C.c_void_p),
        ('lat_trace', C.c_void_p), ('occupancy', C.c_void_p), ('steps_done', C.c_void_p),
        ('last_exp', C.c_void_p),
        ('n', C.c_int32), ('trial_cap', C.c_int32), ('instance_base', C.c_uint32),
        ('flags', C.c_uint32), ('trials_target', C.c_int32), ('steps_per_trial', C.c_int32),
        ('step_budget', C.c_int32),
        ('alpha', C.c_double), ('gamma', C.c_double), ('epsilon', C.c_double),
        ('seed', C.c_uint64),
        ('param_sets', C.c_void_p), ('param_index', C.c_void_p), ('n_param_sets', C.c_int32),
        ('mon_stripes', C.c_int32),
        ('traffic', C.c_void_p),
    ]


_P = C.c_void_p
_SIGNATURES = {
    'cobel_last_error': (C.c_char_p, []),
    'cobel_abi_version': (C.c_int, []),
    'cobel_rng_uniform': (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_int32,
                                    C.c_int32, _P]),
    'cobel_rng_bounded': (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _P,
                                    C.c_int32, C.c_int32, C.c_int32, _P]),
    'cobel_rng_bounded_each': (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P,
                                         C.c_int32, C.c_int32, C.c_int32, _P]),
    'cobel_eps_greedy_f64': (C.c_int, [_P, _P, _P, C.c_double, _P, _P, C.c_int32, _P]),
    'cobel_world_create': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(_P)]),
    'cobel_world_create_n': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.POINTER(_P)]),
    'cobel_world_actions': (C.c_int, [_P, C.POINTER(C.c_int32)]),
    'cobel_world_destroy': (C.c_int, [_P]),
    'cobel_world_info': (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32)]),
    'cobel_world_set_transitions': (C.c_int, [_P, _P, _P, _P, C.c_int64]),
    'cobel_world_update': (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    'cobel_world_update_transitions': (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    'cobel_env_step': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_uint32, _P]),
    'cobel_env_step_draw': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int32, C.c_uint32,
                                      _P]),
    'cobel_env_reset': (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_int32, C.c_uint32, _P]),
    'cobel_gather_rows': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    'cobel_eps_greedy': (C.c_int, [_P, _P, _P, C.c_double, _P, _P, C.c_int32, _P]),
    'cobel_eps_greedy_n': (C.c_int, [_P, _P, _P, C.c_double, _P, _P, C.c_int32, C.c_int32, _P]),
    'cobel_eps_greedy_n_f64': (C.c_int, [_P, _P, _P, C.c_double, _P, _P, C.c_int32, C.c_int32,
                                         _P]),
    'cobel_param_set_fill': (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.POINTER(ParamSet)]),
    'cobel_sfma_param_set_fill': (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double,
                                            C.POINTER(C.c_double * 10), C.POINTER(SFMAParamSet)]),
    'cobel_tab_query': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32)]),
    'cobel_tab_run': (C.c_int, [_P, C.POINTER(TabRun), _P]),
    'cobel_dynaq_run': (C.c_int, [_P, C.POINTER(TabRun), _P]),
    'cobel_q_run': (C.c_int, [_P, C.POINTER(TabRun), _P]),
    'cobel_tab_describe': (C.c_int, [_P, C.POINTER(TabRun), C.POINTER(C.c_int32)]),
    'cobel_tab_scratch_check': (C.c_int, [_P, C.c_int64, _P]),
    'cobel_tab_policy_run': (C.c_int, [_P, C.POINTER(TabPolicyRun), _P]),
    'cobel_tab_policy_plan': (C.c_int, [_P, C.POINTER(TabPolicyRun), C.POINTER(C.c_int32 * 4)]),
    'cobel_policy_select_n': (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32,
                                        C.c_int32, _P]),
    'cobel_dynaq_replay': (C.c_int, [_P, C.POINTER(TabRun), C.c_int32, _P]),
    'cobel_dynaq_replay_plan': (C.c_int, [_P, C.POINTER(TabRun), C.c_int32,
                                          C.POINTER(C.c_int32 * 4)]),
    'cobel_dynaq_update': (C.c_int, [_P, C.POINTER(TabRun), _P, C.c_uint32, _P, _P]),
    'cobel_model_store': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_double, _P]),
    'cobel_tab_rollout': (C.c_int, [_P, C.POINTER(TabRollout), _P]),
    'cobel_tab_rollout_plan': (C.c_int, [_P, C.POINTER(TabRollout), C.POINTER(C.c_int32 * 4)]),
    'cobel_rollout_visits': (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_uint32,
                                       _P, _P]),
    'cobel_pack_model': (C.c_uint64, [C.c_float, C.c_uint16, C.c_uint8]),
    'cobel_unpack_model': (None, [C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint16),
                                  C.POINTER(C.c_uint8)]),
    'cobel_model_init': (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    'cobel_model_index_build': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    'cobel_pairwise_order': (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    'cobel_sr_init': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P]),
    'cobel_sr_run': (C.c_int, [_P, C.POINTER(SRRun), _P]),
    'cobel_sr_retrieve_q': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    'cobel_sfma_query': (C.c_int, [C.c_int32, C.POINTER(C.c_int32)]),
    'cobel_sfma_plan': (C.c_int, [C.c_int32, C.c_uint32, C.POINTER(C.c_int32 * 4)]),
    'cobel_sfma_exp_check': (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_void_p]),
    'cobel_sfma_run': (C.c_int, [_P, C.POINTER(SFMARun), _P]),
    'cobel_sfma_mem_plan': (C.c_int, [C.c_int32, C.c_uint32, C.POINTER(C.c_int32 * 4)]),
    'cobel_sfma_store': (C.c_int, [C.POINTER(SFMAMem), _P, _P]),
    'cobel_sfma_replay': (C.c_int, [C.POINTER(SFMAMem), C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                    _P]),
    'cobel_sfma_random_batch': (C.c_int, [C.POINTER(SFMAMem), C.c_int32, _P, _P, _P]),
    'cobel_pma_param_set_fill': (C.c_int, [C.POINTER(C.c_double * 7), C.c_double, C.c_double,
                                           C.c_double, C.POINTER(PMAParamSet)]),
    'cobel_pma_update_q_sets': (C.c_int, [C.POINTER(PMAMem), _P, _P, _P, C.c_int32, C.c_int64,
                                          C.c_int32, _P, _P]),
    'cobel_pma_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]),
    'cobel_pma_plan_wide': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]),
    'cobel_pma_replay': (C.c_int, [C.POINTER(PMAMem), C.c_int32, _P, _P, _P, _P, _P]),
    'cobel_pma_trial': (C.c_int, [_P, C.POINTER(PMAMem), C.POINTER(PMARun), _P]),
    'cobel_pma_store': (C.c_int, [C.POINTER(PMAMem), _P, _P]),
    'cobel_pma_update_sr': (C.c_int, [C.POINTER(PMAMem), _P]),
    'cobel_pma_stationary': (C.c_int, [C.POINTER(PMAMem), _P, _P, _P, _P]),
    'cobel_pma_plan_need': (C.c_int, [C.c_int32, C.POINTER(C.c_int32 * 2)]),
    'cobel_pma_stationary_wide': (C.c_int, [C.POINTER(PMAMem), _P, _P, _P, _P, C.c_int64, _P]),
    'cobel_pma_plan_need_wide': (C.c_int, [C.c_int32, C.POINTER(C.c_int64 * 4)]),
    'cobel_pma_gain_batch': (C.c_int, [C.POINTER(PMAMem), _P, C.c_int64, _P, _P]),
    'cobel_pma_gain_seq': (C.c_int, [C.POINTER(PMAMem), _P, C.c_int64, _P, _P, C.c_int32,
                                     C.c_int32, C.c_int64, _P, _P]),
    'cobel_pma_action_probs': (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_double, _P, _P]),
    'cobel_pma_update_q': (C.c_int, [C.POINTER(PMAMem), _P, _P, _P, C.c_int32, C.c_int64,
                                     C.c_double, _P, C.c_int32, _P]),
    'cobel_metric_sr': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_double, _P, _P]),
    'cobel_metric_dr': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                  _P, _P, C.c_int64, _P]),
    'cobel_metric_plan': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64 * 4)]),
    'cobel_mfec_pairs': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    'cobel_mfec_run': (C.c_int, [_P, C.POINTER(MFECMem), C.POINTER(MFECRun), _P]),
    'cobel_mfec_estimate': (C.c_int, [C.POINTER(MFECMem), _P, C.c_int32, _P, _P]),
    'cobel_rw_plan': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]),
    'cobel_rw_run': (C.c_int, [C.POINTER(Seq), C.POINTER(RWRun), _P]),
    'cobel_rw_predict': (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P]),
    'cobel_seq_step': (C.c_int, [C.POINTER(Seq), _P, _P, _P, _P, _P, _P]),
    'cobel_seq_reset': (C.c_int, [C.POINTER(Seq), _P, _P]),
    'cobel_qseq_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]),
    'cobel_qseq_run': (C.c_int, [C.POINTER(Seq), C.POINTER(QSeqRun), _P]),
    'cobel_softmax_n': (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    'cobel_anet_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]),
    'cobel_anet_run': (C.c_int, [C.POINTER(Seq), C.POINTER(ANetRun), _P]),
    'cobel_anet_predict': (C.c_int, [C.POINTER(ANetRun), C.c_int32, _P, C.c_int32, _P, _P]),
    'cobel_anet_update': (C.c_int, [C.POINTER(ANetRun), C.c_int32, _P, _P, _P, _P]),
    'cobel_adqn_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64 * 4)]),
    'cobel_adqn_store': (C.c_int, [C.POINTER(ADQNMem), C.c_int32, _P, _P, _P, _P]),
    'cobel_adqn_sample': (C.c_int, [C.POINTER(ADQNMem), C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'cobel_adqn_step': (C.c_int, [C.POINTER(Seq), C.POINTER(ADQNMem), C.POINTER(ADQNStep), _P]),
    'cobel_adam_step': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P,
                                  C.c_double, _P]),
}
_SIGNATURES['cobel_dqn_replay_query'] = (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32)])
_SIGNATURES['cobel_dqn_replay'] = (C.c_int, [C.POINTER(DQNReplay), _P])
_SIGNATURES['cobel_dqn_act'] = (C.c_int, [_P, C.POINTER(DQNAct), _P])
_SIGNATURES['cobel_mlp_query'] = (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32)])
_SIGNATURES['cobel_mlp_forward'] = (C.c_int, [C.POINTER(MLPForward), _P])
_SIGNATURES['cobel_mlp_fit'] = (C.c_int, [C.POINTER(MLPFit), _P])
_SIGNATURES['cobel_mlp_activity'] = (C.c_int, [C.POINTER(MLPActivity), _P])
_SIGNATURES['cobel_activity_process'] = (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32,
                                                   C.c_double, _P])
_SIGNATURES['cobel_place_fields_plan'] = (C.c_int, [C.c_int32, C.c_int32, C.c_int32,
                                                    C.POINTER(C.c_int32 * 4)])
_SIGNATURES['cobel_place_fields'] = (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_double, C.c_double, _P, _P, _P, _P, _P, _P])
_SIGNATURES['cobel_dsr_targets'] = (C.c_int, [C.POINTER(DSRTargets), _P])
_SIGNATURES['cobel_c2d_plan'] = (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)])
_SIGNATURES['cobel_c2d_step'] = (C.c_int, [C.POINTER(C2D), _P, _P, _P, _P, _P])
_SIGNATURES['cobel_c2d_reset'] = (C.c_int, [C.POINTER(C2D), _P, _P, _P])
_SIGNATURES['cobel_dqn_act_c2d'] = (C.c_int, [C.POINTER(DQNActC2D), _P])
EXPORTS = tuple(sorted(_SIGNATURES))

_lib = None


def lib() -> C.CDLL:
    """Load the shared library once; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'libcobel_hip.so is missing (%s): build it with '
                '`make -C cobel-rl_amd/csrc` or `python -c "import __graft_entry__ as g; '
                'g.build()"` — there is no CPU fallback' % LIB_PATH)
        # torch ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  The process must
        # end up with ONE HIP runtime, the one that owns torch's allocations and streams, so
        # torch is loaded first and the library's NEEDED entry binds to that copy.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int) -> None:
    """Map library status codes onto the exceptions the reference would raise."""
    if rc == OK:
        return
    msg = lib().cobel_last_error().decode('utf-8', 'replace')
    if rc == E_ARG:
        raise AssertionError(msg)
    if rc == E_RANGE:
        raise IndexError(msg)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise CobelHipError(msg)


def ptr(t) -> int | None:
    """Device (or host) address of a torch tensor / numpy array, None for None."""
    if t is None:
        return None
    if hasattr(t, 'data_ptr'):
        assert t.is_contiguous(), 'tensor handed to the C ABI must be contiguous'
        return t.data_ptr()
    assert t.flags['C_CONTIGUOUS']
    return t.ctypes.data


def current_stream(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
