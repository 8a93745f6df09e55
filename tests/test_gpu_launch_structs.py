"""What the agents' launchers hand to the library: the run struct of every fused agent, recorded at
the library entry, names the tensors and carries the scalars of its session — in per-step callback
mode (one instance, ``step_budget`` 1, ``last_exp`` set) and vectorised (4 096 instances, striped
monitors, action mask, response counts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, BASE = 0xC0BE1, 3
# agent -> (library entry, position of the run struct among its arguments)
ENTRY = {'QAgent': ('cobel_q_run', 1), 'DynaQ': ('cobel_dynaq_run', 1), 'SR': ('cobel_sr_run', 1),
         'SFMA': ('cobel_sfma_run', 1), 'PMA': ('cobel_pma_trial', 2)}
PARAMS = ('recency_tab', 'recency_len', 'model_lr', 'decay_inhibition', 'decay_strength', 'c_step',
          'i_step', 'r_threshold', 'beta', 'reward_modulation', 'blend', 'interp_fwd', 'interp_rev')


def fields_of(struct) -> dict:
    return {f[0]: getattr(struct, f[0]) for f in struct._fields_}


def record(monkeypatch, entry: str, position: int, calls: list, expect=None) -> None:
    """Pass-through recorder on a library entry: the fields of the struct at ``position`` and, taken
    at the same moment, what ``expect()`` says they should be."""
    from cobel_amd import _lib
    real = getattr(_lib.lib(), entry)

    def through(*args):
        calls.append((fields_of(args[position]._obj), expect() if expect else None,
                      [a._obj for a in args if hasattr(a, '_obj')]))
        return real(*args)

    monkeypatch.setattr(_lib.lib(), entry, through)


def make(kind: str, n_envs: int, callbacks=None):
    from cobel_amd import agent as agents
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory, SFMAMemory
    from cobel_amd.misc.gridworld_tools import make_open_field
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(make_open_field(5, 5, 0, 1), n_envs=n_envs, seed=SEED, instance_base=BASE)
    spaces, pol = (env.observation_space, env.action_space), EpsilonGreedy(0.1)
    if kind == 'SFMA':
        xy = np.asarray(env.world['coordinates'], dtype=np.float64)
        D = np.exp(-np.linalg.norm(xy[:, None, :] - xy[None, :, :], axis=2))
        mem = SFMAMemory(D, 25, 4, decay_inhibition=0.8, decay_strength=0.95, learning_rate=0.7)
        mem.recency, mem.deterministic, mem.beta, mem.blend = True, True, 9, 0.3
        mem.C_step, mem.I_step, mem.R_threshold, mem.reward_modulation = 1.5, 0.75, 1e-5, 2.0
        mem.interpolation_fwd, mem.interpolation_rev = 0.25, 0.625
        agent = agents.SFMA(*spaces, pol, mem, custom_callbacks=callbacks)
        agent.random = True
    elif kind == 'PMA':
        mem = PMAMemory(env.world['sas'], EpsilonGreedy(0.1))
        agent = agents.PMA(*spaces, pol, mem, custom_callbacks=callbacks)
    else:
        agent = getattr(agents, kind)(*spaces, pol, custom_callbacks=callbacks)
    return env, agent


def expectation(env, agent, per_step: bool):
    """The tensors the struct must name and the scalars that follow the agent, at call time."""
    def expect():
        mon = agent.monitors
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        want = {k: ptr(mon.raw(k)) for k in ('lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt')}
        want.update(lat_trace=ptr(mon.lat_trace), occupancy=ptr(mon.occupancy),
                    steps_done=ptr(mon.steps_done), trial_cap=mon.cap, mon_stripes=mon.stripes,
                    inst=ptr(agent.inst), action_mask=ptr(agent._mask_dev),
                    last_exp=ptr(agent._last_exp) if per_step else None)
        if per_step:
            want['trials_target'] = agent.current_trial + 1
        return want
    return expect


def check(calls, session: dict, declared_only=()):
    assert calls, 'the library entry was never reached'
    for got, want, _ in calls:
        want = dict(want, **session)
        for name in declared_only:
            if name not in got:
                want.pop(name, None)
        for name, value in want.items():
            assert name in got, '%s is no field of the struct' % name
            assert got[name] == value, (name, got[name], value)
        assert got['lat_sum'] and got['lat_cnt'] and got['reward_sum'] and got['steps_done']
        assert got['inst']


# (cobel_pma_run_t: the mask, the instance count, the seed and the trial target travel elsewhere)
PMA_LACKS = ('action_mask', 'last_exp', 'n', 'instance_base', 'seed', 'trials_target', 'step_budget')


@pytest.mark.parametrize('kind', sorted(ENTRY))
def test_per_step_launches_name_last_exp(monkeypatch, kind):
    """One instance with an ``on_step_end`` callback: a launch per env step with ``step_budget``
    1 and ``last_exp`` set (PMA fires no step callbacks and launches per trial)."""
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    seen = []
    env, agent = make(kind, 1, {'on_step_end': [lambda logs: seen.append(logs.get('step'))]})
    calls = []
    record(monkeypatch, *ENTRY[kind], calls, expectation(env, agent, kind != 'PMA'))
    trials, steps = 2, 4
    if kind in ('QAgent', 'SR'):
        agent.train(env, trials, steps)
    else:
        agent.train(env, trials, steps, 8)
    session = dict(n=1, instance_base=BASE, seed=SEED, steps_per_trial=steps, step_budget=1,
                   mon_stripes=1, trial_cap=trials, action_mask=None, resp_cnt=None,
                   lat_trace=None, occupancy=None)
    check(calls, session, PMA_LACKS if kind == 'PMA' else ())
    if kind == 'PMA':
        assert len(calls) == trials and not seen
    else:
        assert len(calls) == len(seen) >= trials and all(c[0]['last_exp'] for c in calls)
        assert [c[0]['trials_target'] for c in calls] == sorted(c[0]['trials_target'] for c in calls)
        assert {c[0]['trials_target'] for c in calls} == {1, 2}


@pytest.mark.parametrize('kind', sorted(ENTRY))
def test_vectorised_launch_names_stripes_mask_and_responses(monkeypatch, kind):
    """4 096 instances (the stripes switch on), 2 trials x 10 steps, action mask and response
    counts on: one launch for the whole session (PMA: one per trial), ``last_exp`` NULL."""
    import torch
    from cobel_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    n, trials, steps = 4096, 2, 10
    env, agent = make(kind, n)
    agent.mask_actions = agent.track_responses = agent.track_instances = True
    agent.action_mask[7, 2] = False
    calls = []
    record(monkeypatch, *ENTRY[kind], calls, expectation(env, agent, False))
    if kind in ('QAgent', 'SR'):
        agent.train(env, trials, steps)
    else:
        agent.train(env, trials, steps, 8)
    session = dict(n=n, instance_base=BASE, seed=SEED, steps_per_trial=steps, step_budget=0,
                   trials_target=trials, mon_stripes=16, trial_cap=trials, last_exp=None,
                   occupancy=None)
    check(calls, session, PMA_LACKS if kind == 'PMA' else ())
    assert len(calls) == (trials if kind == 'PMA' else 1)
    for got, _, structs in calls:
        assert got['resp_cnt'] and got['lat_trace']
        assert agent.monitors.raw('resp_cnt').shape == (16, trials)
        if kind == 'PMA':       # the mask is a member of cobel_pma_mem_t
            mem = fields_of(structs[0])
            assert mem['action_mask'] == agent._mask_dev.data_ptr()
            assert (mem['n'], mem['instance_base'], mem['seed']) == (n, BASE, SEED)
        else:
            assert got['action_mask'] == agent._mask_dev.data_ptr()
        assert got['flags'] & _lib.F_MASK_ACTIONS and got['flags'] & _lib.F_LEARN
    bits = agent._mask_dev.cpu().numpy()
    assert bits.dtype == np.uint8 and bits[7] == 0b1011 and (np.delete(bits, 7) == 15).all()
    torch.cuda.synchronize()

    if kind == 'SFMA':
        # the parameter block of a store() on the memory is the one train() passed, field by field
        run = calls[0][0]
        stores = []
        record(monkeypatch, 'cobel_sfma_store', 0, stores)
        agent.M.store({'state': 0, 'action': 1, 'reward': 0.5, 'next_state': 1, 'terminal': 1})
        mem = stores[0][0]
        for name in PARAMS:
            assert mem[name] == run[name], name
        M = agent.M
        assert run['recency_tab'] == M._recency_table(agent.device).data_ptr() and run['recency_len'] > 1
        assert [run[k] for k in PARAMS[2:]] == [0.7, 0.8, 0.95, 1.5, 0.75, 1e-5, 9.0, 2.0, 0.3, 0.25,
                                                0.625]
        own = _lib.SF_RANDOM | _lib.SF_DYNAMIC | _lib.SF_START_REPLAY
        assert run['sfma_flags'] & own == _lib.SF_RANDOM
        assert mem['sfma_flags'] == run['sfma_flags'] & ~own == (
            _lib.SF_DETERMINISTIC | _lib.SF_RECENCY | _lib.SF_R_NORMALIZE)
        assert (mem['n'], mem['instance_base'], mem['seed']) == (n, BASE, SEED)
