"""The argument checks of both C ABIs that need a live handle: exact return code and exact so100_last_error() bytes (recorded from the
library before the host layer under the two ABIs was unified), and after each failure the handle still works and the caller's current
device is what it was.  Every call here is rejected on the host before any launch."""
import ctypes as C

import pytest
import torch

INVALID = -1


@pytest.mark.gpu
def test_rejected_calls_leave_code_message_and_a_working_handle():
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.collector import RolloutCollector
    import gpu_support as G

    n, T = 16, 2
    sim = lib.So100Sim(1, n, flags=lib.F_CUBE_PINNED)
    learner = lib.So100Learner(15, max_minibatch=64)
    L, dev, od = sim.L, sim.device, sim.obs_dim
    stream = sim._stream()
    sim.set_policy(G.policy_tensors(RolloutCollector.random_policy_state(od, dev, seed=0)))
    sim.reset()

    f = dict(dtype=torch.float32, device=dev)
    act = torch.zeros(n, 6, **f)
    buf = torch.zeros(T, n, od + 10, **f)
    params = torch.zeros(learner.num_params, **f)
    adam_m, adam_v = torch.zeros_like(params), torch.zeros_like(params)
    adv, ret, adv_stats, stats = torch.zeros(T, n, **f), torch.zeros(T, n, **f), torch.zeros(2, **f), torch.zeros(4, **f)
    row = torch.zeros(n, **f)
    p = lambda t: t.data_ptr()

    def step_io(**over):
        kw = dict(act_dev=p(act), obs_dev=p(sim.obs), rew_dev=p(sim.rew), done_dev=p(sim.done), trunc_dev=p(sim.trunc))
        kw.update(over)
        return lib.StepIO(**kw)

    def rollout_io():
        return lib.RolloutIO(rollout_dev=p(buf), obs_dev=p(sim.obs), rew_dev=p(sim.rew), done_dev=p(sim.done), trunc_dev=p(sim.trunc))

    def adv_io(**over):
        kw = dict(rollout_dev=p(buf), last_obs_dev=p(sim.obs), params_dev=p(params), adv_dev=p(adv), ret_dev=p(ret), adv_stats_dev=p(adv_stats))
        kw.update(over)
        return lib.AdvantagesIO(**kw)

    def mb_io(**over):
        kw = dict(rollout_dev=p(buf), num_samples=T * n, idx_dev=None, mb=T * n, adam_step=1, adv_dev=p(adv), ret_dev=p(ret), adv_stats_dev=p(adv_stats),
                  params_dev=p(params), adam_m_dev=p(adam_m), adam_v_dev=p(adam_v), stats_dev=p(stats))
        kw.update(over)
        return lib.MinibatchIO(**kw)

    weights_one_null = lib.PolicyWeights.from_buffer_copy(sim._pw)
    weights_one_null.vf_w1 = None
    pio = lib.PolicyIO(obs_dev=None, act_env_dev=p(act))

    sim_calls = [
        (lambda: L.so100_step(sim.h, C.byref(step_io(act_dev=None)), stream), b"so100_step: act/obs/rew/done/trunc pointers are required"),
        (lambda: L.so100_rollout(sim.h, C.byref(sim._pw), C.byref(rollout_io()), 0, 0, stream), b"so100_rollout: T must be >= 1"),
        (lambda: L.so100_rollout(sim.h, C.byref(weights_one_null), C.byref(rollout_io()), T, 0, stream), b"so100_rollout: null weight pointer"),
        (lambda: L.so100_policy_forward(sim.h, C.byref(sim._pw), C.byref(pio), 0, stream), b"so100_policy_forward: obs and act_env pointers are required"),
        (lambda: L.so100_get_field(sim.h, -1, p(row), stream), b"so100_get_field: bad argument"),
        (lambda: L.so100_get_field(sim.h, 98, p(row), stream), b"so100_get_field: bad argument"),
    ]
    learner_calls = [
        (lambda: L.so100_learner_advantages(learner.h, C.byref(adv_io()), 0, n, stream), b"so100_learner_advantages: T must be >= 1, got 0"),
        (lambda: L.so100_learner_advantages(learner.h, C.byref(adv_io()), T, 0, stream), b"so100_learner_advantages: N must be >= 1, got 0"),
        (lambda: L.so100_learner_advantages(learner.h, C.byref(adv_io(adv_dev=None)), T, n, stream),
         b"so100_learner_advantages: rollout/last_obs/params/adv/ret/adv_stats pointers are required"),
        (lambda: L.so100_learner_minibatch_step(learner.h, C.byref(mb_io(mb=0)), stream),
         b"so100_learner_minibatch_step: mb must be in 1..max_minibatch, got 0"),
        (lambda: L.so100_learner_minibatch_step(learner.h, C.byref(mb_io(mb=65)), stream),
         b"so100_learner_minibatch_step: mb must be in 1..max_minibatch, got 65"),
        (lambda: L.so100_learner_minibatch_step(learner.h, C.byref(mb_io(adam_step=0)), stream),
         b"so100_learner_minibatch_step: adam_step is 1-based, got 0"),
    ]
    assert L.so100_num_state_fields() == 98            # index 98 is the first one past the end
    current = torch.cuda.current_device()
    for call, msg in sim_calls + learner_calls:
        assert call() == INVALID, msg
        assert L.so100_last_error() == msg
        # the same handles go on working: a reset, one step, one advantages pass over a 2 x 16 chunk
        sim.reset()
        sim.step(act)
        learner.advantages(buf, sim.obs, params, adv, ret, adv_stats)
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert torch.isfinite(sim.obs).all() and torch.isfinite(adv).all()
    sim.close(); learner.close()
