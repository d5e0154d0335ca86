"""Slots on different weight versions in one policy launch (actor/batched.py ``n_sets``, the kernels' ``MIX``
variants, actor/vec.py ``league_step='mixed'``).

* the set plan (``build_set_plan``): every slot once, grouped by set and ascending inside a set, -1 pads, unused
  trailing tiles, the tile bound, out-of-range indices refused;
* ``TorchSlotPolicy(n_sets=3)``: every active slot is stepped by its own set's weights, also after a reset moved it;
* ``VecActor(league_step='mixed')`` on the CPU: the league bookkeeping of the separate step, ONE policy step per
  group step, no opponent policies, ``h_set`` = 1 + the game's opponent index on the opponent slots;
* on the GPU: a mixed step is BITWISE what three single-version policies of the same class compute for the slots of
  their set (actions, log-probabilities, values, masks, LSTM state), graph-captured and eager, over a schedule with
  inactive slots, slots that move between sets with a reset, and empty sets; edge splits; ``n_sets=1`` is the
  policy built without the argument; a hot swap of one set leaves the others' slots bit-identical; the runtime's
  rollouts replay under the eager policy.
"""
import random

import numpy as np
import pytest
import torch

from dotaclient_amd import native
from dotaclient_amd.actor.batched import TorchSlotPolicy, build_set_plan, plan_tiles
from dotaclient_amd.models.policy import Policy, get_config, masked_log_softmax

needs_native = pytest.mark.skipif(not native.AVAILABLE, reason='native module not built')


# ---------------------------------------------------------------------------------------------------- the set plan
def _check_plan(h, n_sets, even):
    n = len(h)
    T = plan_tiles(n, n_sets, even=even)
    assert T >= (n + 15 * n_sets) // 16 and T <= (n + 15 * n_sets) // 16 + 1
    rows = np.full(16 * T, 12345, np.int32)
    tile_set = np.full(T, 12345, np.int32)
    used = build_set_plan(h, n_sets, rows, tile_set)
    assert used <= (n + 15 * n_sets) // 16 <= T                        # the tile count is within T
    valid = rows[rows >= 0]
    assert sorted(valid.tolist()) == list(range(n))                    # every slot exactly once
    assert set(rows[rows < 0].tolist()) <= {-1}                        # pads are -1
    assert np.all(tile_set[used:] == -1) and np.all(tile_set[:used] >= 0)     # trailing tiles unused
    assert np.all(rows[16 * used:] == -1)
    assert np.all(np.diff(tile_set[:used]) >= 0)                       # grouped by set, sets ascending
    for t in range(used):
        r = rows[16 * t:16 * t + 16]
        k = int((r >= 0).sum())
        assert k >= 1 and np.all(r[:k] >= 0) and np.all(r[k:] == -1)   # pads only at a tile's end
        assert np.all(h[r[:k]] == tile_set[t])                         # a tile's rows share its set
        if k < 16:                                                     # a partial tile ends its set's run
            assert t == used - 1 or tile_set[t + 1] != tile_set[t]
    for s in range(n_sets):
        mine = np.concatenate([rows[16 * t:16 * t + 16] for t in range(used) if tile_set[t] == s] or
                              [np.zeros(0, np.int32)])
        mine = mine[mine >= 0]
        assert mine.tolist() == np.flatnonzero(h == s).tolist()        # ascending slot order within a set (stable)


@pytest.mark.parametrize('n', [1, 15, 16, 17, 33, 40])
@pytest.mark.parametrize('n_sets', [1, 2, 3])
def test_set_plan_properties(n, n_sets):
    rng = np.random.default_rng(100 * n + n_sets)
    for even in (False, True):
        for _ in range(4):
            _check_plan(rng.integers(0, n_sets, n).astype(np.int32), n_sets, even)
        for s in range(n_sets):                                        # everything in one set
            _check_plan(np.full(n, s, np.int32), n_sets, even)


@pytest.mark.parametrize('bad', [-1, 3, 1 << 20])
def test_set_plan_refuses_out_of_range_indices(bad):
    n, n_sets = 40, 3
    T = plan_tiles(n, n_sets)
    h = np.arange(n, dtype=np.int32) % n_sets
    h[17] = bad
    with pytest.raises(ValueError):
        build_set_plan(h, n_sets, np.zeros(16 * T, np.int32), np.zeros(T, np.int32))
    with pytest.raises(ValueError):                                    # too few tiles for the assignment
        build_set_plan(np.arange(n, dtype=np.int32) % n_sets, n_sets, np.zeros(16 * 2, np.int32),
                       np.zeros(2, np.int32))


# ------------------------------------------------------------------------------------------- the eager slot policy
def _policies(cfg, k=3, seed=10):
    out = []
    for i in range(k):
        torch.manual_seed(seed + i)
        out.append(Policy(cfg).eval())
    return out


def _observations(cfg, n, seed):
    rng = np.random.default_rng(seed)
    U = cfg.layout.max_units
    env = rng.standard_normal((n, 3)).astype(np.float32)
    units = rng.standard_normal((n, U, 10)).astype(np.float32)
    handles = np.where(rng.random((n, U)) < 0.5, rng.integers(1, 1000, (n, U)), -1).astype(np.int64)
    handles[:, 0] = 1
    return env, units, handles


def test_torch_slot_policy_steps_each_slot_on_its_set():
    cfg = get_config('lstm128')
    pols = _policies(cfg)
    with torch.no_grad():
        for k, p in enumerate(pols):                                   # value bands 100·k apart
            p.affine_value.weight.mul_(0.01)
            p.affine_value.bias.fill_(100.0 * k)
    n = 12
    sp = TorchSlotPolicy(pols[0], n, n_sets=3)
    for k in (1, 2):
        sp.load_weights(pols[k], set=k)
    with pytest.raises(ValueError):
        sp.load_weights(pols[0], set=3)
    env, units, handles = _observations(cfg, n, 0)
    sp.h_env.copy_(torch.from_numpy(env)); sp.h_units.copy_(torch.from_numpy(units))
    sp.h_handles.copy_(torch.from_numpy(handles))
    hs = (np.arange(n) % 3).astype(np.int32)
    active = np.ones(n, np.float32)
    active[[2, 7]] = 0.0
    sp.h_set.numpy()[:] = hs
    sp.h_active.numpy()[:] = active
    sp.step_async()
    out = sp.wait()
    on = active > 0
    assert np.all(np.abs(out['value'][on] - 100.0 * hs[on]) < 20.0)
    assert np.all(out['value'][~on] == 0.0) and not np.any(sp.h[~on])  # inactive: not stepped
    # the single-set policy of set k gives the same values for set k's slots
    for k in range(3):
        one = TorchSlotPolicy(pols[k], n)
        one.h_env.copy_(sp.h_env); one.h_units.copy_(sp.h_units); one.h_handles.copy_(sp.h_handles)
        one.h_active.numpy()[:] = active
        one.step_async()
        sel = on & (hs == k)
        np.testing.assert_allclose(out['value'][sel], one.wait()['value'][sel], atol=1e-5)
    # slots reset and reassigned follow their new set
    moved = np.array([0, 4, 8])
    hs2 = hs.copy()
    hs2[moved] = (hs[moved] + 1) % 3
    sp.h_set.numpy()[:] = hs2
    sp.h_keep.numpy()[moved, 0] = 0.0
    sp.h_active.numpy()[:] = 1.0
    sp.step_async()
    out = sp.wait()
    assert np.all(np.abs(out['value'] - 100.0 * hs2) < 20.0)
    sp.h_set.numpy()[3] = 5                                            # an index no set has: refused
    with pytest.raises(ValueError):
        sp.step_async()
    with pytest.raises(ValueError):
        TorchSlotPolicy(pols[0], n, n_sets=2, inputs_from=sp)


# -------------------------------------------------------------------------------------------------- the runtime
HEADS = [('enum', 0, 3), ('x', 3, 9), ('y', 12, 9)]


def _store(cfg, versions=(0,), seed=0):
    from dotaclient_amd.actor.weights import WeightStore
    ws = WeightStore(cfg, device='cpu')
    for v in versions:
        torch.manual_seed(seed + v)
        ws.add(v, {k: t.detach().clone() for k, t in Policy(cfg).state_dict().items()})
    return ws


def _replay(policy, r, stride):
    """Re-run a rollout under the eager policy from its first stored LSTM state: (states at the stride points,
    values, logp of the recorded actions)."""
    r.ensure_units()
    U = r.units.shape[1]
    heads = HEADS + [('target_unit', 21, U)]
    h = (torch.from_numpy(r.hiddens[0, 0].copy())[None, None], torch.from_numpy(r.hiddens[0, 1].copy())[None, None])
    hs, vals, lps = [], [], []
    with torch.no_grad():
        for t in range(r.length):
            if t % stride == 0:
                hs.append(np.stack([h[0][0, 0].numpy(), h[1][0, 0].numpy()]))
            logits, value, h = policy.forward_packed(torch.from_numpy(r.env[t:t + 1].copy())[None],
                                                     torch.from_numpy(r.units[t:t + 1].copy())[None], h)
            vals.append(float(value[0, 0, 0]))
            lp = 0.0
            for k, o, w in heads:
                m = torch.from_numpy(r.masks[t, o:o + w].astype(bool))
                if not m.any():
                    continue
                a = int(np.argmax(r.actions[t, o:o + w]))
                lp += float(masked_log_softmax(logits[k].reshape(1, w).float(), m[None], dim=-1)[0, a])
            lps.append(lp)
    return np.stack(hs), np.array(vals, np.float32), np.array(lps, np.float32)


@needs_native
def test_vec_actor_mixed_league_step_cpu():
    """The existing league test's settings with league_step='mixed'."""
    from dotaclient_amd.actor.league import League
    from dotaclient_amd.actor.vec import VecActor
    from dotaclient_amd.transport.codec import decode
    cfg = get_config('lstm128')
    ws = _store(cfg, versions=(0, 1, 2))
    league = League(ws, mode='uniform', rng=random.Random(0))
    sent = []
    va = VecActor(ws, 4, sent.append, device='cpu', seed=9, max_dota_time=15.0, hidden_stride=8, threads=2,
                  groups=2, latest_weights_prob=0.0, league=league, opponent_refresh=2, league_step='mixed')
    assert all(isinstance(g.gp, TorchSlotPolicy) and g.gp.n_sets == 3 for g in va.groups)
    # spies: policy steps per group step, and the staged h_set against the game's opponent index
    launches = {'observe': 0, 'steps': 0}
    seen_opponent_sets = set()
    for g in va.groups:
        def spy(snapshot_rows=None, g=g, inner=g.gp.step_async):
            launches['steps'] += 1
            hset = g.gp.h_set.numpy()
            opp = np.asarray(g.ve.opponent_slots(), dtype=np.int64)
            want = np.zeros(g.S, np.int32)
            want[opp] = 1 + g.game_opp[opp // g.ppg]
            assert np.array_equal(hset, want)
            assert np.all(want[opp] >= 1) and np.all(want[opp] <= 2)
            seen_opponent_sets.update(want[opp].tolist())
            return inner(snapshot_rows=snapshot_rows)
        g.gp.step_async = spy
    inner_launch = va._observe_and_launch

    def count(g):
        launches['observe'] += 1
        return inner_launch(g)
    va._observe_and_launch = count
    while va.games_finished < 6:
        va.step()
    assert launches['steps'] == launches['observe'] > 0                # ONE policy step per group step
    assert seen_opponent_sets == {1, 2}                                # both snapshot sets were played (rotation)
    teams = {}
    for b in sent:
        r = decode(b)
        teams.setdefault(r.game_id, set()).add(r.team_id)
    assert teams and all(len(t) == 1 for t in teams.values())
    assert sum(g for _, g in league.stats().values()) == va.opp_games_finished == va.games_finished
    assert all(len(g.opp) <= 2 and all(o.gp is None for o in g.opp) for g in va.groups)   # no opponent policies
    # hot swap: a new latest version reaches the games started after it, which replay exactly under it
    torch.manual_seed(99)
    ws.add(7, {k: t.detach().clone() for k, t in Policy(cfg).state_dict().items()})
    n0 = va.games_finished
    while va.games_finished < n0 + 4:
        va.step()
    sent.clear()
    while va.games_finished < n0 + 8:
        va.step()
    rs = [decode(b) for b in sent]
    assert rs and all(r.weight_version == 7 for r in rs)
    pol = ws.policy_for(ws.latest_weights())
    for r in rs:
        _, vals, lps = _replay(pol, r, 8)
        np.testing.assert_allclose(vals, r.values, atol=2e-5)
        np.testing.assert_allclose(lps, r.logp, atol=5e-4)


@needs_native
def test_vec_actor_league_step_argument_is_checked():
    from dotaclient_amd.actor.vec import VecActor
    ws = _store(get_config('lstm128'))
    with pytest.raises(ValueError):
        VecActor(ws, 2, None, device='cpu', league_step='fused')


# ------------------------------------------------------------------------------------------------------ GPU
def _policy_class(precision):
    from dotaclient_amd.actor.batched import F32ActorPolicy, Fp8ActorPolicy, GpuActorPolicy
    return {'bf16': GpuActorPolicy, 'fp32': F32ActorPolicy, 'fp8': Fp8ActorPolicy}[precision]


def _step(gp, obs, reset, active, h_set=None):
    if h_set is not None:
        gp.h_set.numpy()[:] = h_set
    out = gp.step(*obs, reset=reset, active=active)
    torch.cuda.synchronize()
    out = {k: np.array(v) for k, v in out.items()}
    out['h'], out['c'] = gp.h.cpu().numpy(), gp.c.cpu().numpy()
    return out


def _assert_mixed_equals_refs(m, refs, h_set, active, tag):
    on = np.asarray(active, bool)
    for k, ref in enumerate(refs):
        mine = h_set == k
        for name in ('idx', 'logp', 'value', 'actions', 'masks'):
            a, b = m[name][mine & on], ref[name][mine & on]
            assert a.tobytes() == b.tobytes(), (tag, name, k)
        for name in ('h', 'c'):
            assert m[name][mine].tobytes() == ref[name][mine].tobytes(), (tag, name, k)


def _schedule(n):
    """(h_set, reset, active) of the four steps: thirds; some slots inactive; a third of the slots reset into another
    set; everything reset into set 2 (two empty sets, trailing tiles unused)."""
    i = np.arange(n)
    s0 = (i % 3).astype(np.int32)
    none, all_on = np.zeros(n, bool), np.ones(n, bool)
    off = all_on.copy()
    off[[1, 5, 6, 17, n - 1]] = False
    moved = i % 3 == 1
    s2 = s0.copy()
    s2[moved] = (s0[moved] + 1 + (i[moved] // 3) % 2) % 3
    return [(s0, none, all_on), (s0, none, off), (s2, moved, all_on), (np.full(n, 2, np.int32), all_on, all_on)]


def _run_against_refs(precision, preset, n, schedule, graph):
    cls = _policy_class(precision)
    cfg = get_config(preset)
    pols = _policies(cfg)
    mixed = cls(pols[0], n, device='cuda', seed=7, use_graph=graph, n_sets=3)
    for k in (1, 2):
        mixed.load_weights(pols[k], set=k)
    refs = [cls(p, n, device='cuda', seed=7, use_graph=graph) for p in pols]
    for t, (h_set, reset, active) in enumerate(schedule):
        obs = _observations(cfg, n, 50 + t)
        m = _step(mixed, obs, reset, active, h_set)
        outs = [_step(r, obs, reset, active) for r in refs]
        _assert_mixed_equals_refs(m, outs, h_set, active, (precision, preset, graph, t))
    # the three sets do compute different things (else the comparison above shows nothing)
    assert not np.array_equal(outs[0]['value'], outs[2]['value'])


MIXED_CASES = [(p, s) for p in ('fp32', 'bf16') for s in ('lstm512', 'lstm128', 'compat')] + [('fp8', 'lstm512')]


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('precision,preset', MIXED_CASES)
def test_mixed_step_bitwise_equals_single_version_steps(gpu_ops, precision, preset, graph):
    _run_against_refs(precision, preset, 40, _schedule(40), graph)


@pytest.mark.gpu
@pytest.mark.parametrize('split', [(16, 16, 8), (1, 38, 1)])
@pytest.mark.parametrize('precision,preset', [('fp32', 'lstm128'), ('bf16', 'lstm128'), ('fp8', 'lstm512')])
def test_mixed_step_edge_splits(gpu_ops, precision, preset, split):
    n = sum(split)
    h_set = np.repeat(np.arange(3), split).astype(np.int32)
    perm = np.random.default_rng(3).permutation(n)
    h_set = h_set[perm]                                                # the sets' slots interleaved
    none, all_on = np.zeros(n, bool), np.ones(n, bool)
    _run_against_refs(precision, preset, n, [(h_set, none, all_on), (h_set, none, all_on)], False)


@pytest.mark.gpu
@pytest.mark.parametrize('precision,preset', [('fp32', 'lstm128'), ('bf16', 'lstm128'), ('fp8', 'lstm512')])
def test_one_set_is_the_policy_without_the_argument(gpu_ops, precision, preset):
    cls = _policy_class(precision)
    cfg = get_config(preset)
    pol = _policies(cfg, 1)[0]
    n = 40
    a = cls(pol, n, device='cuda', seed=7, use_graph=False, n_sets=1)
    b = cls(pol, n, device='cuda', seed=7, use_graph=False)
    assert not hasattr(a, 'h_set') and a.w['bpre'].shape == b.w['bpre'].shape
    active = np.ones(n, bool)
    active[[3, 9]] = False
    for t in range(2):
        obs = _observations(cfg, n, 80 + t)
        oa, ob = _step(a, obs, None, active), _step(b, obs, None, active)
        for name in oa:
            assert oa[name].tobytes() == ob[name].tobytes(), name


@pytest.mark.gpu
def test_mixed_policy_refuses_what_it_does_not_cover(gpu_ops):
    from dotaclient_amd.actor.batched import GpuActorPolicy
    pol = _policies(get_config('lstm128'), 1)[0]
    base = GpuActorPolicy(pol, 16, device='cuda', use_graph=False)
    with pytest.raises(ValueError):
        GpuActorPolicy(pol, 16, device='cuda', use_graph=False, n_sets=2, inputs_from=base)
    with pytest.raises(ValueError):
        GpuActorPolicy(_policies(get_config('5v5'), 1)[0], 16, device='cuda', use_graph=False, n_sets=2)
    gp = GpuActorPolicy(pol, 16, device='cuda', use_graph=False, n_sets=2)
    with pytest.raises(ValueError):
        gp.load_weights(pol, set=2)
    gp.h_set.numpy()[5] = 2                                            # no such set: refused before any launch
    with pytest.raises(ValueError):
        gp.step_async()


@pytest.mark.gpu
@pytest.mark.parametrize('precision,preset', [('bf16', 'lstm512'), ('fp8', 'lstm512'), ('fp32', 'lstm128')])
def test_hot_swap_of_one_set_after_capture(gpu_ops, precision, preset):
    cls = _policy_class(precision)
    cfg = get_config(preset)
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
    # a single-version policy of the new weights, from the same state and sampler counter
    one = cls(pols[3], n, device='cuda', seed=7, use_graph=False)
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


@needs_native
@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_vec_actor_gpu_mixed_league_step_replay_consistent(gpu_ops, precision):
    """The lstm512 league test of the GPU runtime with league_step='mixed'."""
    from dotaclient_amd.actor.batched import GpuActorPolicy
    from dotaclient_amd.actor.league import League
    from dotaclient_amd.actor.vec import VecActor
    from dotaclient_amd.transport.codec import decode
    cfg = get_config('lstm512')
    ws = _store(cfg, versions=(0, 1))
    sent = []
    va = VecActor(ws, 16, sent.append, device='cuda', seed=3, rollout_size=32, max_dota_time=20.0, mode='1v1',
                  hidden_stride=16, threads=4, groups=2, latest_weights_prob=0.5,
                  league=League(ws, mode='uniform', rng=random.Random(1)), precision=precision,
                  league_step='mixed')
    assert all(isinstance(g.gp, GpuActorPolicy) and g.gp.n_sets == 3 for g in va.groups)
    while va.games_finished < 24:
        va.step()
    va.close()
    assert va.opp_games_finished > 0
    assert all(o.gp is None for g in va.groups for o in g.opp)
    pol = ws.policy_for(ws.latest_weights())
    rs = [decode(b) for b in sent]
    assert len(rs) > 16
    assert all(r.units is None and r.units_raw is not None and r.hero is not None for r in rs)
    for r in rs[:60]:
        hs, vals, lps = _replay(pol, r, 16)
        np.testing.assert_allclose(hs, r.hiddens, atol=5e-2)
        np.testing.assert_allclose(vals, r.values, atol=5e-2)
        np.testing.assert_allclose(lps, r.logp, atol=1e-1)
