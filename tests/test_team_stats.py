"""Recurrence telemetry, host half (ops/lstm.py decoder, learner/optimizer.py metrics, learner/e2e.py result fields).

A statistics block holds one 64-byte record per team-recurrence launch (which XCD teams committed / aborted / never
arrived, chains per team, device time of the call) in a ring of the 64 most recent launches of its stream, plus running
totals; the learner turns the blocks into ``team/*`` metrics without a host sync. These tests decode blocks built by
hand from the documented layout (the kernels do not write one yet, profiles/team_telemetry.md). Nothing here sets
DCA_TEAM_FAIL or makes a hand-off time out."""
import numpy as np
import pytest
import torch

from dotaclient_amd.ops import lstm as L
from dotaclient_amd.ops.lstm import parse_team_stats


# ------------------------------------------------------------------------------------------------------------------
# CPU: the decoder against the documented layout
# ------------------------------------------------------------------------------------------------------------------
def _put_record(w, seq, kind=0, nch=8, err=0, committed=0xff, aborted=0, absent=0, chains=(1,) * 8, ticks=1000,
                qticks=10):
    r = w[L.STAT_HDR_WORDS + L.STAT_REC_WORDS * ((seq - 1) % L.STAT_RING):][:L.STAT_REC_WORDS]
    r[:] = 0
    r[1], r[2], r[3] = kind, nch, err
    r[4] = committed | (aborted << 8) | (absent << 16)
    for x, c in enumerate(chains):
        r[5 + x // 2] |= c << (16 * (x % 2))
    r[9], r[10] = ticks & 0xffffffff, ticks >> 32
    r[11], r[12] = qticks & 0xffffffff, qticks >> 32
    r[0] = seq


def test_parse_wrapped_ring_and_degraded_record():
    w = np.zeros(L.STAT_WORDS, np.uint32)
    for seq in range(1, 71):                                  # 70 launches: slots 0..5 are overwritten by 65..70
        _put_record(w, seq, kind=seq % 2, ticks=100 * seq)
    # launch 70: XCD 3's leader timed out, team 0 ran its chain
    _put_record(w, 70, kind=0, nch=8, committed=0b11110111, aborted=0b00001000, chains=(2, 1, 1, 0, 1, 1, 1, 1),
                ticks=250_000, qticks=123_456)
    w[0] = 70
    fwd = w[L.STAT_KIND_BASE:]
    fwd[0], fwd[2], fwd[3] = 35, 1, 1
    big = (7 << 32) + 12345                                   # a tick sum above 2^32
    fwd[7], fwd[8] = big & 0xffffffff, big >> 32
    fwd[9], fwd[10] = 250_000, 0
    bwd = w[L.STAT_KIND_BASE + L.STAT_KIND_WORDS:]
    bwd[0], bwd[5], bwd[6] = 35, 280, 0
    for block in (w, w.view(np.int32), torch.from_numpy(w.view(np.int32).copy())):
        p = parse_team_stats(block)
        assert p['seq'] == 70 and p['lost'] == 6
        assert [r['seq'] for r in p['records']] == list(range(7, 71))
        assert [r['kind'] for r in p['records'][:3]] == ['bwd', 'fwd', 'bwd']
        last = p['records'][-1]
        assert last['committed'] == [0, 1, 2, 4, 5, 6, 7] and last['aborted'] == [3] and last['absent'] == []
        assert last['chains'] == [2, 1, 1, 0, 1, 1, 1, 1] and last['nch'] == 8 and last['degraded'] is True
        assert last['ms'] == 2.5 and last['queue_ms'] == 1.23456 and last['err'] == 0
        assert not any(r['degraded'] for r in p['records'][:-1])
        assert p['records'][0]['ms'] == 700 / 1e5
        assert p['fwd']['launches'] == 35 and p['fwd']['degraded'] == 1 and p['fwd']['aborted'] == 1
        assert p['fwd']['ticks'] == big and p['fwd']['ms_sum'] == big / 1e5 and p['fwd']['ms_max'] == 2.5
        assert p['bwd']['launches'] == 35 and p['bwd']['chains'] == 280 and p['bwd']['ticks'] == 0
    with pytest.raises(ValueError):
        parse_team_stats(np.zeros(100, np.uint32))
    empty = parse_team_stats(np.zeros(L.STAT_WORDS, np.uint32))
    assert empty['records'] == [] and empty['lost'] == 0 and empty['fwd']['launches'] == 0


def test_parse_absent_team_and_more_chains_than_teams():
    w = np.zeros(L.STAT_WORDS, np.uint32)
    # 10 chains on 8 teams: two chains on two of them is the even spread (ceil(10 / 8) = 2), three is not
    _put_record(w, 1, nch=10, chains=(2, 2, 1, 1, 1, 1, 1, 1))
    _put_record(w, 2, kind=1, nch=10, committed=0x7f, absent=0x80, chains=(3, 2, 1, 1, 1, 1, 1, 0))
    w[0] = 2
    a, b = parse_team_stats(w)['records']
    assert a['degraded'] is False and b['degraded'] is True
    assert b['absent'] == [7] and b['committed'] == list(range(7)) and b['kind'] == 'bwd'


def test_summary_p99_and_unchanged_keys():
    from dotaclient_amd.learner.e2e import _summary
    rng = np.random.default_rng(0)
    rows = [tuple(rng.uniform(0.5, 2.0, 17)) for _ in range(40)]
    rows[7] = rows[7][:10] + (22.6,) + rows[7][11:]             # one outlier iteration
    rows[9] = rows[9][:10] + (float('nan'),) + rows[9][11:]
    cfg = dict(seq_per_epoch=16, seq_len=1400)
    s = _summary(rows, 12.5, 1000, 3, 64, cfg)
    a = np.asarray(rows, dtype=np.float64)
    assert s['learner_gpu_ms_per_step_p99'] == float(np.nanpercentile(a[:, 10], 99))
    assert s['learner_gpu_ms_per_step'] == float(np.nanmean(a[:, 10]))
    assert s['learner_gpu_ms_per_step_max'] == 22.6
    # every key of the summary as it was before the p99 was added keeps its value
    want = {
        'steps_per_s': 40 * 16 * 1400 / 12.5, 'valid_steps_per_s': float(a[:, 5].sum()) / 12.5, 'iterations': 40,
        'wall_s': 12.5, 'avg_weight_age': float(a[:, 1].mean()), 'avg_rollout_len': float(a[:, 2].mean()),
        'train_ms_per_iteration': 1e3 * float(a[:, 3].mean()), 'ingest_ms_per_iteration': 1e3 * float(a[:, 4].mean()),
        'h2d_ms_per_iteration': 1e3 * float(a[:, 6].mean()), 'log_ms_per_iteration': 1e3 * float(a[:, 7].mean()),
        'publish_ms_per_iteration': 1e3 * float(a[:, 8].mean()),
        'lookahead_ms_per_iteration': 1e3 * float(a[:, 9].mean()), 'rollouts_consumed': int(np.nansum(a[:, 11])),
        'stage_ms_per_iteration': 1e3 * float(np.nanmean(a[:, 12])),
        'gather_ms_per_iteration': 1e3 * float(np.nanmean(a[:, 13])),
        'stage_wait_ms_per_iteration': 1e3 * float(np.nanmean(a[:, 14])),
        'stage_copy_ms_per_iteration': 1e3 * float(np.nanmean(a[:, 15])),
        'stage_release_ms_per_iteration': 1e3 * float(np.nanmean(a[:, 16])), 'actor_steps_per_s': 1000 / 12.5,
        'queue_dropped': 3, 'games': 64, 'config': cfg,
    }
    for k, v in want.items():
        assert s[k] == v, k
    assert set(s) == set(want) | {'learner_gpu_ms_per_step', 'learner_gpu_ms_per_step_max',
                                  'learner_gpu_ms_per_step_p99'}
    none = _summary([], 1.0, 0, 0, 1, cfg)
    assert np.isnan(none['learner_gpu_ms_per_step_p99'])


def _rollout(i, T=32):
    from dotaclient_amd.constants import LAYOUT_1V1
    from dotaclient_amd.transport.codec import Rollout
    rng = np.random.default_rng(i)
    U, A = LAYOUT_1V1.max_units, 21 + LAYOUT_1V1.max_units
    act = np.zeros((T, A), np.uint8)
    act[:, 0] = 1
    msk = np.zeros((T, A), np.uint8)
    msk[:, :3] = 1
    return Rollout(game_id=f'g{i}', team_id=2 + i % 2, player_id=0, weight_version=0,
                   env=rng.standard_normal((T, 3)).astype(np.float32),
                   units=rng.standard_normal((T, U, 10)).astype(np.float32), actions=act, masks=msk,
                   rewards=rng.standard_normal((T, 9)), logp=np.full(T, -1.0, np.float32),
                   values=np.zeros(T, np.float32), done=True)


def _optimizer(tmp_path, device, **kw):
    from dotaclient_amd.learner.optimizer import DotaOptimizer, OptimizerConfig
    from dotaclient_amd.transport.broker import InProcBroker
    from dotaclient_amd.transport.codec import encode
    br = InProcBroker()
    for i in range(16):
        br.publish_experience(encode(_rollout(i)))
    cfg = OptimizerConfig(log_dir=str(tmp_path), model='lstm128', epochs=1, seq_per_epoch=4, batch_size=2, seq_len=32,
                          device=device, xp_timeout=30, **kw)
    return DotaOptimizer(cfg, br)


def test_cpu_torch_iteration_has_no_team_metrics(tmp_path):
    opt = _optimizer(tmp_path, 'cpu')
    opt.run(iterations=1)
    assert opt.learner.backend == 'torch' and opt.learner.team_stat_tensors() == []
    assert np.isfinite(opt.last_metrics['loss/sum'])
    assert not [k for k in opt.last_metrics if k.startswith('team/')]


def test_team_window_fields():
    from dotaclient_amd.learner.e2e import _team_add, _team_window
    acc = {}
    _team_add(acc, {'loss/sum': 1.0})                          # (an iteration without telemetry adds nothing)
    assert _team_window(acc) == {}
    base = {'team/launches': 4.0, 'team/degraded': 0.0, 'team/aborted': 0.0, 'team/absent': 0.0, 'team/fwd_ms': 2.0,
            'team/bwd_ms': 3.0, 'team/fwd_ms_max': 2.5, 'team/bwd_ms_max': 3.5, 'team/queue_ms_max': 0.01,
            'team/records_lost': 0.0}
    _team_add(acc, base)
    _team_add(acc, dict(base, **{'team/degraded': 1.0, 'team/aborted': 1.0, 'team/fwd_ms': 4.0, 'team/fwd_ms_max': 22.0}))
    assert _team_window(acc) == {'team_launches': 8, 'team_degraded_launches': 1, 'team_aborted': 1, 'team_absent': 0,
                                 'recurrence_fwd_ms': 3.0, 'recurrence_bwd_ms': 3.0, 'recurrence_fwd_ms_max': 22.0,
                                 'recurrence_bwd_ms_max': 3.5}


def _block(launches):
    """A statistics block after ``launches`` = [(kind, ticks, chains, aborted mask)], eight chains each."""
    w = np.zeros(L.STAT_WORDS, np.uint32)
    for seq, (kind, ticks, chains, aborted) in enumerate(launches, 1):
        _put_record(w, seq, kind=kind, nch=8, committed=0xff & ~aborted, aborted=aborted, chains=chains, ticks=ticks,
                    qticks=1000 + seq)
        t = w[L.STAT_KIND_BASE + L.STAT_KIND_WORDS * kind:]
        t[0] += 1
        t[2] += int(max(chains) > 1)
        t[3] += bin(aborted).count('1')
        t[5] += sum(chains)
        t[7] += ticks                                          # (small sums: no carry into word 8 here)
        t[9] = max(int(t[9]), ticks)
        w[0] = seq
    return w


def test_optimizer_team_metrics_from_block_deltas(tmp_path, caplog):
    """``DotaOptimizer._team_metrics``: counts and means from the change of the running totals since the previous
    iteration, maxima from the ring records with a new seq, launches that already left the ring counted as lost, and
    ONE warning line for an iteration with degraded launches."""
    import logging
    opt = _optimizer(tmp_path, 'cpu')
    caplog.clear()                                              # (the constructor's own warnings)
    even = (1,) * 8
    first = [(0, 200_000, even, 0), (1, 220_000, even, 0), (0, 210_000, even, 0), (1, 230_000, even, 0)]
    with caplog.at_level(logging.WARNING, logger='dotaclient_amd.learner.optimizer'):
        m = opt._team_metrics([_block(first)], 1)
    assert m == {'team/launches': 4.0, 'team/degraded': 0.0, 'team/aborted': 0.0, 'team/absent': 0.0,
                 'team/fwd_ms': 2.05, 'team/bwd_ms': 2.25, 'team/fwd_ms_max': 2.1, 'team/bwd_ms_max': 2.3,
                 'team/queue_ms_max': 0.01004, 'team/records_lost': 0.0}
    assert not caplog.records
    # the next iteration: XCD 3's leader times out in two forward launches (team 0 and team 5 run a second chain)
    second = first + [(0, 1_100_000, (2, 1, 1, 0, 1, 1, 1, 1), 8), (1, 240_000, even, 0),
                      (0, 1_300_000, (1, 1, 1, 0, 1, 2, 1, 1), 8), (1, 250_000, even, 0)]
    with caplog.at_level(logging.WARNING, logger='dotaclient_amd.learner.optimizer'):
        m = opt._team_metrics([_block(second)], 2)
    assert m['team/launches'] == 4.0 and m['team/degraded'] == 2.0 and m['team/aborted'] == 2.0
    assert m['team/fwd_ms'] == 12.0 and m['team/bwd_ms'] == 2.45
    assert m['team/fwd_ms_max'] == 13.0 and m['team/bwd_ms_max'] == 2.5 and m['team/records_lost'] == 0.0
    assert len(caplog.records) == 1                             # one line per iteration, however many launches
    line = caplog.records[0].getMessage()
    assert 'it=2' in line and 'aborted [3]' in line and '13.000 ms' in line and '2 degraded' in line
    # 70 more launches before the next snapshot: 6 of them have already left the ring
    third = second + [(seq % 2, 100_000, even, 0) for seq in range(70)]
    m = opt._team_metrics([_block(third)], 3)
    assert m['team/launches'] == 70.0 and m['team/records_lost'] == 6.0 and m['team/degraded'] == 0.0
    assert m['team/fwd_ms'] == 1.0 and m['team/fwd_ms_max'] == 1.0
