"""Fused MI355X learner path (HIP kernels) vs the fp32 torch reference: loss and every parameter gradient.

Short horizons here (the bf16x3 ``fp32`` learner, and ``fp32-exact``); the deploy horizon (S=1400) is pinned in
test_fp32_kernels.py / test_exact_mode.py. A bf16 learner has no kernel path: it runs on the torch backend."""
import copy

import pytest
import torch

from dotaclient_amd.learner.engine import Learner, LossConfig
from dotaclient_amd.learner.synthetic import make_batch
from dotaclient_amd.models.policy import Policy, get_config

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# (the ids keep the trailing "-1" they had while the step could also run in time chunks, so the cases keep their names)
@pytest.mark.parametrize('preset,algo,B,S', [('lstm512', 'ppo', 4, 48), ('lstm128', 'ppo', 7, 33),
                                             ('compat', 'vpg', 3, 40), ('lstm512', 'vpg', 2, 30),
                                             ('5v5', 'ppo', 3, 24)],
                         ids=['lstm512-ppo-4-48-1', 'lstm128-ppo-7-33-1', 'compat-vpg-3-40-1', 'lstm512-vpg-2-30-1',
                              '5v5-ppo-3-24-1'])
def test_fused_loss_and_grads_match_reference(gpu_ops, preset, algo, B, S):
    torch.manual_seed(0)
    cfg = get_config(preset)
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    lc = LossConfig(algo=algo, vf_coef=0.5, entropy_coef=0.01)
    fused = Learner(pol, lc, device='cuda', backend='fused', dp=False, precision='fp32')
    torch_l = Learner(ref, lc, device='cuda', backend='torch', dp=False, precision='fp32')   # fp32 oracle
    batch = make_batch(B, S, cfg.layout, cfg.hidden if cfg.rnn == 'lstm' else None, device='cuda', seed=3)
    for L in (fused, torch_l):
        L.dp.zero_grad()
    lf, mf = fused.loss(batch)
    lf.backward()
    lr_, mr = torch_l.loss(batch)
    lr_.backward()
    torch.cuda.synchronize()
    assert abs(float(lf.detach()) - float(lr_.detach())) <= 2e-2 * max(1.0, abs(float(lr_))), (float(lf), float(lr_))
    for k in ['policy_loss', 'entropy', 'advantage_loss']:
        assert abs(float(mf[k]) - float(mr[k])) <= 3e-2 * max(0.05, abs(float(mr[k]))), (k, float(mf[k]), float(mr[k]))
    # whole-gradient agreement (bf16x3 operands vs the fp32 oracle), plus a looser per-tensor bound
    assert _rel(fused.flat.grad, torch_l.flat.grad) < (6e-2 if preset == "compat" else 3e-2)
    for name, gf, gr in zip(fused.flat.names, [p.grad for p in fused.flat.params],
                            [p.grad for p in torch_l.flat.params]):
        if gr.norm() < 1e-8:
            assert gf.norm() < 1e-6, name
            continue
        assert _rel(gf, gr) < 1.2e-1, (name, _rel(gf, gr))


@pytest.mark.parametrize('precision', ['fp32', 'fp32-exact'])
def test_fused_train_step_decreases_loss(gpu_ops, precision):
    torch.manual_seed(0)
    cfg = get_config('lstm512')
    L = Learner(Policy(cfg), LossConfig(algo='ppo', learning_rate=3e-4), device='cuda', backend='fused', dp=False,
                precision=precision)
    batch = make_batch(4, 64, cfg.layout, cfg.hidden, device='cuda', seed=1)
    losses = [float(L.train_step(batch)['loss']) for _ in range(8)]
    L.model.check_error()
    assert losses[-1] < losses[0]


@pytest.mark.parametrize('precision', ['fp32', 'fp32-exact'], ids=['1-fp32', '1-fp32-exact'])   # (ids as before)
def test_graph_captured_step_matches_eager(gpu_ops, precision):
    """hipGraph-captured forward+backward (Learner.enable_graph) gives the same parameters as eager steps, also
    across host synchronisations between replays (a stale host-staged buffer in the graph would show up there)."""
    torch.manual_seed(0)
    cfg = get_config('lstm512')
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    lc = LossConfig(algo='ppo')
    a = Learner(pol, lc, device='cuda', backend='fused', dp=False, precision=precision)
    b = Learner(ref, lc, device='cuda', backend='fused', dp=False, precision=precision)
    assert b.enable_graph(warmup=1)
    batches = [make_batch(4, 40, cfg.layout, cfg.hidden, device='cuda', seed=s) for s in range(4)]
    for bt in batches:
        ma = a.train_step(bt)
        mb = b.train_step(bt)
        torch.cuda.synchronize()
        torch.cuda.synchronize()
        torch.testing.assert_close(mb['grad_norm'], ma['grad_norm'], rtol=1e-4, atol=1e-7)
    assert b.graph is not None
    torch.testing.assert_close(b.flat.flat, a.flat.flat, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mb['loss'], ma['loss'], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('preset,precision,B,S,reset', [
    ('lstm512', 'fp32-exact', 3, 24, False),        # one-row recurrence chains
    ('lstm512', 'fp32-exact', 9, 24, False),        # uneven two-row chains
    ('lstm512', 'fp32', 3, 24, False),
    ('lstm512', 'fp32-exact', 3, 24, True),         # packed sequences: episode-start flags
    ('5v5', 'fp32-exact', 2, 16, False)])
def test_forward_logp_value_equals_the_steps_logp(gpu_ops, monkeypatch, preset, precision, B, S, reset):
    """``FusedPolicy.forward_logp_value`` (the learner's policy_old evaluation) runs the training step's own forward
    part: its log-probs are bit-equal to the ones the step returns for the same batch and weights (the second output
    of ``PipelinedPolicyLoss``, batch-major)."""
    from dotaclient_amd.models.pipelined import PipelinedPolicyLoss
    torch.manual_seed(0)
    cfg = get_config(preset)
    L = Learner(Policy(cfg), LossConfig(algo='ppo'), device='cuda', backend='fused', dp=False, precision=precision)
    batch = make_batch(B, S, cfg.layout, cfg.hidden, device='cuda', seed=7)
    if reset:
        flags = torch.zeros(B, S, dtype=torch.uint8)
        flags[0, 0] = flags[0, 9] = flags[1, 5] = flags[2, S - 1] = 1
        batch['reset'] = flags.cuda()
    seen = {}
    apply = PipelinedPolicyLoss.apply

    def spy(*args):
        out = apply(*args)
        seen['logp'] = out[1].detach().clone()
        return out
    monkeypatch.setattr(PipelinedPolicyLoss, 'apply', staticmethod(spy))
    L.loss(batch)
    lp, _ = L.evaluate_sequences(batch, B)
    torch.cuda.synchronize()
    L.model.check_error()
    assert seen['logp'].shape == (B * S,) and lp.shape == (B, S)
    assert torch.isfinite(lp).all() and float(lp.abs().max()) > 0
    assert torch.equal(lp.reshape(B * S), seen['logp'])


@pytest.mark.parametrize('precision', ['fp32', 'fp32-exact'])
def test_direct_replay_step_matches_autograd_step(gpu_ops, precision):
    """The autograd-free direct step fed from the HBM replay (time-major gather inside the captured graph) updates
    the parameters exactly like the autograd Function path on the same minibatch."""
    from dotaclient_amd.learner.replay import HbmReplay
    torch.manual_seed(0)
    cfg = get_config('lstm512')
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    lc = LossConfig(algo='ppo')
    a = Learner(pol, lc, device='cuda', backend='fused', dp=False, precision=precision)
    b = Learner(ref, lc, device='cuda', backend='fused', dp=False, precision=precision)
    assert b.direct() and b.enable_graph(warmup=1)
    rep = HbmReplay(6, 40, cfg.layout, cfg.hidden, 'cuda', seed=5)
    rep.add(make_batch(6, 40, cfg.layout, cfg.hidden, device='cuda', seed=9))
    for step in range(3):
        g_state = rep._g.get_state()
        idx = rep.sample_indices(4)
        rep._g.set_state(g_state)
        batch = rep.gather(idx)
        # a: autograd Function path (loss + backward), b: direct replay path (graph from step 1 on)
        a.dp.zero_grad()
        la, ma = a.loss(batch)
        la.backward()
        a.dp.has_grad.copy_(a.model.grad_mask)
        a.dp.sync()
        ma['grad_norm'] = a.opt.step(a.dp.counts)
        mb = b.train_step_replay(rep, 4)
        torch.cuda.synchronize()
        for k in ('loss', 'policy_loss', 'entropy', 'advantage_loss', 'approx_kl', 'clipfrac', 'grad_norm'):
            torch.testing.assert_close(mb[k], ma[k].detach(), rtol=2e-4, atol=2e-6, msg=f'step {step} {k}')
    torch.testing.assert_close(b.flat.flat, a.flat.flat, rtol=1e-5, atol=1e-6)


def test_loss_prep_kernel_matches_batch_norms(gpu_ops):
    from dotaclient_amd.ops.heads import batch_norms
    cfg = get_config('lstm512')
    batch = make_batch(5, 301, cfg.layout, cfg.hidden, device='cuda', seed=2)
    act = batch['actions'].reshape(-1, batch['actions'].shape[-1]).contiguous()
    ret = batch['ret'].reshape(-1)
    ref = batch_norms(act, ret, False, 301)
    ws = torch.zeros(int(gpu_ops.loss_prep_ws_elems()), dtype=torch.int32, device='cuda')
    out = torch.full((8,), 7.0, device='cuda')
    for _ in range(3):                           # the self-resetting counter must allow repeated launches
        gpu_ops.loss_prep(act, ws, out)
        torch.testing.assert_close(out, ref, rtol=1e-6, atol=0)
    assert int(ws[-1]) == 0


@pytest.mark.parametrize('preset,precision', [('lstm512', 'fp32'), ('lstm512', 'fp32-exact'), ('5v5', 'fp32'),
                                              ('5v5', 'fp32-exact')])
def test_fused_step_is_bitwise_deterministic(gpu_ops, preset, precision):
    """Deterministic-mode check: every reduction on the fused step runs in a fixed order (no float
    atomics), so two learners fed the same replay minibatches end bit-identical."""
    from dotaclient_amd.learner.replay import HbmReplay
    cfg = get_config(preset)
    torch.manual_seed(0)
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    learners = [Learner(p, LossConfig(algo='ppo'), device='cuda', backend='fused', dp=False, precision=precision)
                for p in (pol, ref)]
    reps = []
    for L in learners:
        assert L.enable_graph(warmup=1)
        rep = HbmReplay(6, 48, cfg.layout, cfg.hidden, 'cuda', seed=11)
        rep.add(make_batch(6, 48, cfg.layout, cfg.hidden, device='cuda', seed=4))
        reps.append(rep)
    for _ in range(3):
        ms = [L.train_step_replay(rep, 4) for L, rep in zip(learners, reps)]
    torch.cuda.synchronize()
    assert torch.equal(learners[0].flat.flat, learners[1].flat.flat)
    assert torch.equal(ms[0]['loss'], ms[1]['loss']) and torch.equal(ms[0]['grad_norm'], ms[1]['grad_norm'])


@pytest.mark.parametrize('preset,precision', [('lstm512', 'fp32-exact'), ('5v5', 'fp32')])
def test_dp_split_step_matches_single_graph(gpu_ops, monkeypatch, preset, precision):
    """The data-parallel split step (two captured graphs around the point where the recurrence / pre-RNN / heads
    gradients are final, early buckets all-reduced in between) computes exactly what the single-graph step does."""
    from dotaclient_amd.learner.replay import HbmReplay
    cfg = get_config(preset)
    torch.manual_seed(0)
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    flats, losses = [], []
    for p, split in ((pol, '1'), (ref, '0')):
        monkeypatch.setenv('DCA_DP_SPLIT', split)
        L = Learner(p, LossConfig(algo='ppo'), device='cuda', backend='fused', dp=False, precision=precision)
        assert L.enable_graph(warmup=1)
        rep = HbmReplay(6, 48, cfg.layout, cfg.hidden, 'cuda', seed=11)
        rep.add(make_batch(6, 48, cfg.layout, cfg.hidden, device='cuda', seed=4))
        for _ in range(3):
            m = L.train_step_replay(rep, 4)
        torch.cuda.synchronize()
        assert L._split == (split == '1')
        flats.append(L.flat.flat.clone())
        losses.append(m['loss'].clone())
    assert torch.equal(flats[0], flats[1])
    assert torch.equal(losses[0], losses[1])


def _pg_worker(port, q):
    import os
    import torch.distributed as dist
    try:
        # DCA_DP_SPLIT=1: the two-graph split capture (thread_local mode under the live process group) too
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', DCA_DP_SPLIT='1')
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
        t = torch.ones(4, device='cuda')
        dist.all_reduce(t)                      # the RCCL watchdog now tracks work while we capture below
        from dotaclient_amd.learner.replay import HbmReplay
        cfg = get_config('lstm128')
        L = Learner(Policy(cfg), LossConfig(algo='ppo'), device='cuda', backend='fused')
        assert L.enable_graph(warmup=1)
        rep = HbmReplay(4, 32, cfg.layout, cfg.hidden, 'cuda', seed=1)
        rep.add(make_batch(4, 32, cfg.layout, cfg.hidden, device='cuda', seed=2))
        for _ in range(4):
            m = L.train_step_replay(rep, 2)
            dist.all_reduce(t)
        torch.cuda.synchronize()
        q.put(('ok', float(m['loss']), L.graph is not None and L._split))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put(('err', repr(e), False))


def test_graph_capture_with_rccl_process_group(gpu_ops):
    """The captured learner step coexists with an initialised RCCL process group (its watchdog thread runs during
    capture) — the multi-GPU bench path, rehearsed with one rank on the one available GPU."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_pg_worker, args=(port, q))
    p.start()
    res = q.get(timeout=240)
    p.join(timeout=60)
    assert res[0] == 'ok', res
    assert res[2] and res[1] == res[1]


@pytest.mark.parametrize('precision', ['fp32', 'fp32-exact'])
def test_team_formation_failure_never_reaches_the_weights(gpu_ops, monkeypatch, precision):
    """DCA_TEAM_FAIL=1: no workgroup joins a recurrence team, so every chain is left unprocessed. The kernel flags
    err = 3 (checked by its last workgroup), the flag rides in the count-carrying all-reduce bucket, and the fused
    Adam skips the step on the device — parameters, moments and step counts unchanged — before check_error raises
    at the host boundary (reference: NaN check raises before optimizer.step(), optimizer.py:674-676)."""
    cfg = get_config('lstm128')
    torch.manual_seed(0)
    L = Learner(Policy(cfg), LossConfig(algo='ppo'), device='cuda', backend='fused', dp=False, precision=precision)
    batch = make_batch(4, 24, cfg.layout, cfg.hidden, device='cuda', seed=1)
    L.train_step(batch)                                   # a healthy step first
    torch.cuda.synchronize()
    L.model.check_error()
    before = (L.flat.flat.clone(), L.opt.exp_avg.clone(), L.opt.steps.clone())
    monkeypatch.setenv('DCA_TEAM_FAIL', '1')
    L.train_step(batch)
    torch.cuda.synchronize()
    assert int(L.model.err.item()) == 3
    assert torch.equal(L.flat.flat, before[0]) and torch.equal(L.opt.exp_avg, before[1])
    assert torch.equal(L.opt.steps, before[2])
    with pytest.raises(RuntimeError, match='error code 3'):
        L.model.check_error()


def test_iteration_pool_growth_releases_captured_graphs(gpu_ops):
    """The optimizer's per-iteration pool grows twice with graph capture on: each growth releases the graphs bound to
    the old storage (no stale graph can be replayed at a reused address), every graph key has its own static index
    buffer, and the captured steps on the new pools match eager steps on the same minibatches."""
    from dotaclient_amd.learner.optimizer import _IterationPool
    torch.manual_seed(0)
    cfg = get_config('lstm128')
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    lc = LossConfig(algo='ppo')
    a = Learner(pol, lc, device='cuda', backend='fused', dp=False)
    b = Learner(ref, lc, device='cuda', backend='fused', dp=False)
    assert b.direct() and b.enable_graph(warmup=0)
    S = 24
    pool = None
    for cap, seed in ((4, 1), (8, 2), (16, 3)):
        data = make_batch(cap, S, cfg.layout, cfg.hidden, device='cuda', seed=seed)
        fields = {k: v for k, v in data.items() if k in Learner.STEP_FIELDS + ('h0', 'c0')}
        if pool is not None:
            n_before = len(b.graphs)
            assert b.release_graphs(pool) >= 1
            assert len(b.graphs) < n_before
        pool = _IterationPool(fields, cap, S)
        for k in fields:
            pool.data[k].copy_(fields[k])
        for step in range(3):
            idx = torch.randperm(cap, device='cuda')[:4]
            ma = a.train_step_indices(pool, idx)      # eager (a has no graph)
            mb = b.train_step_indices(pool, idx)      # captured from its second call on
            torch.cuda.synchronize()
            torch.testing.assert_close(mb['loss'], ma['loss'], rtol=1e-5, atol=1e-7, msg=f'cap {cap} step {step}')
        torch.testing.assert_close(b.flat.flat, a.flat.flat, rtol=1e-5, atol=1e-6)
    keys = [k for k in b.graphs if k[0] == 'replay']
    index_owners = {k for k in b.graphs if isinstance(b.graphs.static(k), torch.Tensor)}
    assert len(keys) == 1 and index_owners == set(keys)


def test_graph_cache_keeps_static_inputs_per_key(gpu_ops):
    """Captured batch steps of two shapes, interleaved (A, A, B, A, B): every key replays over its own static inputs,
    so a step of shape A after B's capture still equals the eager step (one shared input set would be rebound to
    B's buffers by B's capture, and A's next batch copied into them)."""
    torch.manual_seed(0)
    cfg = get_config('lstm128')
    pol = Policy(cfg)
    ref = copy.deepcopy(pol)
    lc = LossConfig(algo='ppo')
    a = Learner(pol, lc, device='cuda', backend='fused', dp=False)
    b = Learner(ref, lc, device='cuda', backend='fused', dp=False)
    assert b.enable_graph(warmup=1)
    shapes = {'A': (3, 24), 'B': (4, 24)}
    for seed, name in enumerate('AABAB'):
        bt = make_batch(*shapes[name], cfg.layout, cfg.hidden, device='cuda', seed=seed)
        ma = a.train_step(bt)
        mb = b.train_step(bt)
        torch.cuda.synchronize()
        torch.testing.assert_close(mb['grad_norm'], ma['grad_norm'], rtol=1e-4, atol=1e-7, msg=f'step {seed} {name}')
        torch.testing.assert_close(mb['loss'], ma['loss'], rtol=1e-5, atol=1e-6, msg=f'step {seed} {name}')
    torch.testing.assert_close(b.flat.flat, a.flat.flat, rtol=1e-5, atol=1e-6)
    keys = [k for k in b.graphs if k[0] == 'batch']
    assert sorted(k[1:3] for k in keys) == sorted(shapes.values())
    statics = [b.graphs.static(k) for k in keys]
    assert len(keys) == 2 and statics[0] is not statics[1]
    for k, st in zip(keys, statics):
        assert tuple(st['env'].shape[:2]) == k[1:3]
    assert not {v.data_ptr() for v in statics[0].values()} & {v.data_ptr() for v in statics[1].values()}


def test_bf16_learner_has_no_fused_branch():
    """The fused step has no vendor-GEMM bf16 branch: ``backend='fused'`` refuses bf16, ``'auto'`` runs it on the
    torch backend (bf16 autocast, the oracle) — CPU-checkable (no kernel is launched)."""
    from dotaclient_amd.models.fused import FusedPolicy
    pol = Policy(get_config('lstm128'))
    fp = FusedPolicy.__new__(FusedPolicy)
    fp.cfg, fp.fp32 = pol.config, False
    fp.fully_fused, fp.attention_fused = True, False
    assert not fp.use_pipeline()
    fp.fp32 = True
    assert fp.use_pipeline()
