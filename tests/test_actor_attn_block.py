"""The actor's inference form of the 5v5 attention block (``attn_block_act``: ops/csrc/attn_block.hip
``attn_block_fwd_f32_kernel<EX, ACT = true>``) and the mixed-version 5v5 policy step built on it.

* the actor form computes bytewise the learner form's E1, pools and argmax, saves nothing, leaves ``x896[:, :128]``
  alone, and with ``row_set`` runs every row on its own weight set; malformed arguments raise before a launch;
* a 5v5 ``F32ActorPolicy`` step allocates less than the learner form's Xn + QKV activations alone;
* ``F32ActorPolicy(n_sets=3)`` on the 5v5 preset is BITWISE three single-version policies (graph and eager, the
  schedule and edge split of tests/test_actor_mixed.py), also across a hot swap of one set;
* what stays refused: the bf16 5v5 mixed step (policy and runtime), out-of-range set indices;
* the runtime's 5v5 league with ``precision='fp32', league_step='mixed'`` replays under the eager policy.
"""
import random

import numpy as np
import pytest
import torch

from dotaclient_amd import native
from dotaclient_amd.models.policy import get_config
from test_actor_mixed import _observations, _policies, _replay, _run_against_refs, _schedule, _step, _store

needs_native = pytest.mark.skipif(not native.AVAILABLE, reason='native module not built')

U, D = 64, 128
TYPE_OFF = [0, 5, 10, 34, 58, 61, 64]                      # the 5v5 layout's unit-type offsets


def _weight_set(gpu_ops, seed, exact):
    """One random weight set of the block in the kernels' operand form: (bout, gamma, beta, wqh, wql, bq, woh, wol)."""
    from dotaclient_amd.models.pipelined import _frag_order
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)   # noqa: E731
    bout, gamma, beta = r(D) * 0.1, 1 + 0.1 * r(D), 0.1 * r(D)
    wq, bq, wo = r(3 * D, D) * D ** -0.5, r(3 * D) * 0.2, r(D, D) * D ** -0.5
    if exact:
        (wqh, wql), (woh, wol) = ((_frag_order(w), w.new_empty(0)) for w in (wq, wo))
    else:
        (wqh, wql), (woh, wol) = (tuple(_frag_order(t) for t in gpu_ops.split_bf16x2(w)) for w in (wq, wo))
    return bout, gamma, beta, wqh, wql, bq, woh, wol


def _e0(n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randn(n * U, D, device='cuda', generator=g) * 1.5 + 0.3


def _learner(gpu_ops, e0, ws, compat):
    """The learner form on one weight set: (e1, x896, arg)."""
    n = e0.shape[0] // U
    x896 = torch.full((n, 896), -7.0, device='cuda')
    arg = torch.full((n, 6, 128), 255, dtype=torch.uint8, device='cuda')
    out = gpu_ops.attn_block_fwd(e0, *ws, TYPE_OFF, x896, arg, compat, 1e-5)
    return out[6], x896, arg


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('exact', [False, True], ids=['bf16x3', 'fp32'])
@pytest.mark.parametrize('compat', [False, True])
def test_actor_form_equals_learner_form(gpu_ops, compat, exact):
    n = 5
    e0, ws = _e0(n, 5), _weight_set(gpu_ops, 6, exact)
    e1_r, x_r, arg_r = _learner(gpu_ops, e0, ws, compat)
    for with_arg in (False, True):
        x896 = torch.full((n, 896), -7.0, device='cuda')
        arg = torch.full((n, 6, 128), 255, dtype=torch.uint8, device='cuda') if with_arg else None
        e1 = gpu_ops.attn_block_act(e0, *ws, TYPE_OFF, x896, compat, 1e-5, arg=arg)
        torch.cuda.synchronize()
        assert e1.shape == (n * U, D) and _same(e1, e1_r)
        assert _same(x896[:, 128:], x_r[:, 128:])
        assert bool((x896[:, :128] == -7.0).all())                    # the env embedding's columns: untouched
        if with_arg:
            assert _same(arg, arg_r)


@pytest.mark.gpu
@pytest.mark.parametrize('exact', [False, True], ids=['bf16x3', 'fp32'])
def test_per_row_weight_sets(gpu_ops, exact):
    n, row_set = 7, [2, 0, 1, 1, 0, 2, 2]
    e0 = _e0(n, 11)
    sets = [_weight_set(gpu_ops, 20 + k, exact) for k in range(3)]
    stacked = [torch.stack(ts).contiguous() for ts in zip(*sets)]
    refs = [_learner(gpu_ops, e0, ws, False) for ws in sets]
    assert not _same(refs[0][0], refs[1][0]) and not _same(refs[1][0], refs[2][0]) and not _same(refs[0][0], refs[2][0])
    rs = torch.tensor(row_set, dtype=torch.int32, device='cuda')
    x896 = torch.zeros(n, 896, device='cuda')
    arg = torch.zeros(n, 6, 128, dtype=torch.uint8, device='cuda')
    e1 = gpu_ops.attn_block_act(e0, *stacked, TYPE_OFF, x896, False, 1e-5, row_set=rs, n_sets=3, arg=arg)
    torch.cuda.synchronize()
    for i, k in enumerate(row_set):
        e1_r, x_r, arg_r = refs[k]
        assert _same(e1.view(n, U, D)[i], e1_r.view(n, U, D)[i]), i
        assert _same(x896[i, 128:], x_r[i, 128:]), i
        assert _same(arg[i], arg_r[i]), i
    # without row_set every row runs on set 0, whatever else is stacked behind it
    e1 = gpu_ops.attn_block_act(e0, *stacked, TYPE_OFF, x896, False, 1e-5, n_sets=3)
    torch.cuda.synchronize()
    assert _same(e1, refs[0][0])

    # malformed arguments raise before any launch
    def call(ws=stacked, row_set=rs, n_sets=3):
        gpu_ops.attn_block_act(e0, *ws, TYPE_OFF, x896, False, 1e-5, row_set=row_set, n_sets=n_sets)
    for j in range(len(stacked)):
        if stacked[j].numel() == 0:                                    # the exact form's empty lo images
            continue
        short = list(stacked)
        short[j] = stacked[j][:2].contiguous()                         # two sets' worth for n_sets = 3
        with pytest.raises(RuntimeError):
            call(ws=short)
    with pytest.raises(RuntimeError):
        call(ws=list(sets[0]))                                         # one set's worth
    with pytest.raises(RuntimeError):
        call(row_set=rs.long())
    with pytest.raises(RuntimeError):
        call(row_set=rs.float())
    with pytest.raises(RuntimeError):
        call(row_set=rs[:6].contiguous())
    with pytest.raises(RuntimeError):
        call(row_set=torch.zeros(n + 1, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError):
        call(row_set=rs.cpu())
    for bad in (0, -1):
        with pytest.raises(RuntimeError):
            call(n_sets=bad)
        with pytest.raises(RuntimeError):
            call(row_set=None, n_sets=bad)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_actor_step_saves_no_activations(gpu_ops):
    """A 5v5 fp32 policy step allocates less than the learner block's Xn + QKV activations alone (64 slots × 64
    units × (128 + 384) fp32 = 8 MiB). From the tensor shapes: the step's transients are the encoder's x896 / emb / arg
    and E1, 4.4 MB; the learner form added Xn, QKV, O, the LayerNorm statistics and the log-sum-exp, 10.6 MB more."""
    from dotaclient_amd.actor.batched import F32ActorPolicy
    n = 64
    cfg = get_config('5v5')
    gp = F32ActorPolicy(_policies(cfg, 1)[0], n, device='cuda', seed=7, use_graph=False)
    none, all_on = np.zeros(n, bool), np.ones(n, bool)
    _step(gp, _observations(cfg, n, 1), none, all_on)                  # warm step
    obs = _observations(cfg, n, 2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    gp.step(*obs, reset=none, active=all_on)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print('step transients (bytes):', extra)
    assert extra < 64 * 64 * (128 + 384) * 4


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
def test_mixed_5v5_step_bitwise_equals_single_version_steps(gpu_ops, graph):
    _run_against_refs('fp32', '5v5', 40, _schedule(40), graph)


@pytest.mark.gpu
def test_mixed_5v5_step_edge_split(gpu_ops):
    split = (1, 38, 1)
    n = sum(split)
    h_set = np.repeat(np.arange(3), split).astype(np.int32)
    h_set = h_set[np.random.default_rng(3).permutation(n)]             # the sets' slots interleaved
    none, all_on = np.zeros(n, bool), np.ones(n, bool)
    _run_against_refs('fp32', '5v5', n, [(h_set, none, all_on), (h_set, none, all_on)], False)


@pytest.mark.gpu
def test_hot_swap_of_one_5v5_set_after_capture(gpu_ops):
    from dotaclient_amd.actor.batched import F32ActorPolicy as cls
    cfg = get_config('5v5')
    pols = _policies(cfg, 4)
    n = 40
    h_set = (np.arange(n) % 3).astype(np.int32)
    none, all_on = np.zeros(n, bool), np.ones(n, bool)
    gps = []
    for _ in range(2):
        gp = cls(pols[0], n, device='cuda', seed=7, use_graph=True, n_sets=3)
        for k in (1, 2):
            gp.load_weights(pols[k], set=k)
        gps.append(gp)
    swapped, plain = gps
    obs = _observations(cfg, n, 90)
    a, b = _step(swapped, obs, none, all_on, h_set), _step(plain, obs, none, all_on, h_set)
    assert swapped.graph is not None
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    swapped.load_weights(pols[3].state_dict(), set=1)                  # after capture: buffers written in place
    one = cls(pols[3], n, device='cuda', seed=7, use_graph=False)      # same state and sampler counter
    torch.cuda.synchronize()
    one.h.copy_(swapped.h); one.c.copy_(swapped.c); one.ctr.copy_(swapped.ctr)
    torch.cuda.synchronize()
    obs = _observations(cfg, n, 91)
    a, b = _step(swapped, obs, none, all_on, h_set), _step(plain, obs, none, all_on, h_set)
    c = _step(one, obs, none, all_on)
    rest = h_set != 1
    for name in a:
        assert a[name][rest].tobytes() == b[name][rest].tobytes(), name      # the other sets: untouched
        assert a[name][~rest].tobytes() == c[name][~rest].tobytes(), name    # set 1: the new weights
    assert np.all(a['value'][~rest] != b['value'][~rest])


@pytest.mark.gpu
def test_5v5_refusals_that_stay(gpu_ops):
    from dotaclient_amd.actor.batched import F32ActorPolicy, GpuActorPolicy
    cfg = get_config('5v5')
    pol = _policies(cfg, 1)[0]
    with pytest.raises(ValueError):
        GpuActorPolicy(pol, 16, device='cuda', use_graph=False, n_sets=2)
    gp = F32ActorPolicy(pol, 16, device='cuda', use_graph=False, n_sets=2)
    with pytest.raises(ValueError):
        F32ActorPolicy(pol, 16, device='cuda', use_graph=False, n_sets=2, inputs_from=gp)
    ctr = int(gp.ctr.item())
    for bad in (2, -1):
        gp.h_set.numpy()[5] = bad                                      # no such set: refused before any launch
        with pytest.raises(ValueError):
            gp.step_async()
    torch.cuda.synchronize()
    assert int(gp.ctr.item()) == ctr                                   # the core kernel bumps it: it never ran
    if native.AVAILABLE:
        from dotaclient_amd.actor.vec import VecActor
        with pytest.raises(ValueError):
            VecActor(_store(cfg), 2, None, mode='5v5', precision='bf16', league_step='mixed', device='cuda')


@needs_native
@pytest.mark.gpu
def test_vec_actor_gpu_mixed_5v5_league_step_replay_consistent(gpu_ops):
    """The 5v5 case of test_vec_actor.py's GPU league test on the IEEE-fp32 actor with league_step='mixed'."""
    from dotaclient_amd.actor.batched import F32ActorPolicy
    from dotaclient_amd.actor.league import League
    from dotaclient_amd.actor.vec import VecActor
    from dotaclient_amd.transport.codec import decode
    cfg = get_config('5v5')
    ws = _store(cfg, versions=(0, 1))
    sent = []
    va = VecActor(ws, 4, sent.append, device='cuda', seed=3, rollout_size=32, max_dota_time=20.0, mode='5v5',
                  hidden_stride=16, threads=4, groups=2, latest_weights_prob=0.5,
                  league=League(ws, mode='uniform', rng=random.Random(1)), precision='fp32', league_step='mixed')
    assert all(isinstance(g.gp, F32ActorPolicy) and g.gp.n_sets == 3 for g in va.groups)
    while va.games_finished < 6:
        va.step()
    va.close()
    assert va.opp_games_finished > 0
    assert all(o.gp is None for g in va.groups for o in g.opp)         # no opponent policy objects
    pol = ws.policy_for(ws.latest_weights())
    rs = [decode(b) for b in sent]
    assert len(rs) > 16
    assert all(r.units is None and r.units_raw is not None and r.hero is not None for r in rs)
    for r in rs[:60]:
        hs, vals, lps = _replay(pol, r, 16)
        np.testing.assert_allclose(hs, r.hiddens, atol=1e-1)
        np.testing.assert_allclose(vals, r.values, atol=5e-2)
        np.testing.assert_allclose(lps, r.logp, atol=1e-1)
