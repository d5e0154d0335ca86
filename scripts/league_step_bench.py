"""VecActor league throughput (player-steps/s) with the opponents stepped separately or in the mixed launch:

    python3 scripts/league_step_bench.py [n_games] [bf16|fp32|fp8] [latest_weights_prob] [separate|mixed|policy] [steps]

Self-play of ``n_games`` games of the ``PRESET`` policy (environment variable; default lstm512, 1v1; ``5v5``: the
entity-attention policy in 5v5 games) against a uniform league over three stored versions; with
``latest_weights_prob`` 0.0 every game has an opponent team (snapshot evaluation, actor/validate.py), 0.8 is BASELINE
config 5. Rollouts are published into a list that is dropped. ``DEVICE=cpu`` runs the eager slot policy. Prints one
JSON line. Run each setting in a fresh process (``separate`` and ``mixed`` alternating) when comparing. ``policy``: the
policy step alone (see :func:`policy_only`); where the policy refuses a mixed step (5v5 below fp32), ``us_mixed`` is
null."""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dotaclient_amd.actor.league import League  # noqa: E402
from dotaclient_amd.actor.vec import VecActor  # noqa: E402
from dotaclient_amd.actor.weights import WeightStore  # noqa: E402
from dotaclient_amd.models.policy import Policy, get_config  # noqa: E402

n_games = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
precision = sys.argv[2] if len(sys.argv) > 2 else 'fp8'
lwp = float(sys.argv[3]) if len(sys.argv) > 3 else 0.8
league_step = sys.argv[4] if len(sys.argv) > 4 else 'separate'
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 1000
warmup = 50
device = torch.device(os.environ.get('DEVICE', 'cuda'))
sync = (lambda: torch.cuda.synchronize(device)) if device.type == 'cuda' else (lambda: None)

preset = os.environ.get('PRESET', 'lstm512')
cfg = get_config(preset)
team = cfg.layout.counts[0]                     # players per team: 1 (1v1 presets) or 5


def policy_only():
    """``policy`` in place of separate|mixed: the policy step of ONE group (n_games slots) without the engine — staged
    copy in → graph replay → copy out, one step at a time: the single-version step, the runtime's separate league
    step (the latest-weights policy and two opponent policies over all slots, as with both snapshots busy) and the
    mixed step with a share (1 − latest_weights_prob) / 2 of the slots on the snapshot sets."""
    import numpy as np
    from dotaclient_amd.actor.batched import make_slot_policy
    torch.manual_seed(0)
    pol = Policy(cfg)
    n, kw = n_games, dict(device=device, precision=precision, raw=True)
    rng = np.random.default_rng(0)

    def fill(gp):
        from dotaclient_amd.features.raw import F_PRESENT
        U = cfg.layout.max_units
        hero = np.zeros((n, 4), np.float32)
        hero[:, :2] = rng.uniform(-7000, 7000, (n, 2))
        hero[:, 2] = 600.0
        raw = np.zeros((n, U, 8), np.int32)
        raw.view(np.float32)[..., :5] = rng.uniform(-1000, 1000, (n, U, 5))
        raw[..., 5] = rng.integers(1, 1000, (n, U))
        raw[..., 6] = np.where(rng.random((n, U)) < 0.6, F_PRESENT, 0)
        gp.stage_raw(rng.standard_normal((n, 3)).astype(np.float32), hero, raw)

    def timed(launch, wait):
        for _ in range(warmup):
            launch(); wait()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            launch(); wait()
        return (time.perf_counter() - t0) / steps * 1e6

    one = make_slot_policy(pol, n, seed=1, **kw)
    fill(one)
    t_single = timed(one.step_async, one.wait)
    opps = [make_slot_policy(pol, n, seed=2 + k, inputs_from=one, **kw) for k in range(2)]

    def launch_sep():
        for o in opps:
            o.step_async()
        one.step_async()

    def wait_sep():
        one.wait()
        for o in opps:
            o.wait()
    t_sep = timed(launch_sep, wait_sep)
    del opps, one
    games = n // (2 * team)                                            # a game's two teams: at most one opponent
    opp = np.flatnonzero(rng.random(games) < 1.0 - lwp)
    hs = np.zeros(n, np.int32)
    first = team * (2 * opp + rng.integers(0, 2, len(opp)))           # first slot of each opponent team
    hs[first[:, None] + np.arange(team)] = rng.integers(1, 3, len(opp))[:, None]
    try:
        mixed = make_slot_policy(pol, n, seed=1, n_sets=3, **kw)
    except ValueError:                                                 # no mixed step for this policy / precision
        t_mixed = None
    else:
        fill(mixed)
        mixed.h_set.numpy()[:] = hs
        t_mixed = timed(mixed.step_async, mixed.wait)
    print(json.dumps({'policy_only': True, 'precision': precision, 'latest_weights_prob': lwp, 'slots': n,
                      'preset': preset,
                      'us_single': t_single, 'us_separate_3_policies': t_sep, 'us_mixed': t_mixed,
                      'slots_per_set': np.bincount(hs, minlength=3).tolist()}))


if league_step == 'policy':
    policy_only()
    sys.exit(0)
ws = WeightStore(cfg, device='cpu')
for v in range(3):
    torch.manual_seed(v)
    ws.add(v, {k: t.detach().clone() for k, t in Policy(cfg).state_dict().items()})
sink = []
va = VecActor(ws, n_games, lambda b: sink.append(len(b)), device=device, seed=1, threads=int(os.environ.get('THREADS', 8)),
              groups=2, hidden_stride=1400, rollout_size=9999, max_dota_time=600.0, stagger=True, precision=precision,
              latest_weights_prob=lwp, league=League(ws, mode='uniform', rng=random.Random(0)),
              opponent_refresh=64, league_step=league_step, mode='5v5' if team > 1 else '1v1')
for _ in range(warmup):
    va.step()
sync()
s0, t0 = va.steps_taken, time.perf_counter()
for _ in range(steps):
    va.step()
sync()
dt = time.perf_counter() - t0
busy = [sum(1 for o in g.opp if o.games > 0) for g in va.groups]
va.close()
print(json.dumps({'league_step': league_step, 'precision': precision, 'latest_weights_prob': lwp, 'games': n_games,
                  'steps_per_s': (va.steps_taken - s0) / dt, 'ms_per_step': dt / steps * 1e3,
                  'busy_opponents_per_group': busy, 'opp_games_finished': va.opp_games_finished}))
