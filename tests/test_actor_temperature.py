"""Per-slot sampling temperature and greedy action selection of the actor.

``sample_kernel<TEMP = true>`` (ops/csrc/actor.hip) takes one τ per row: τ > 0 samples every head from the masked
softmax of (logit − max) / τ and reports the log-prob under that tempered distribution; otherwise the row is greedy —
the arg-max of the masked raw logits, lowest index on ties, no RNG call, log-prob 0. Checked here

* on the GPU: τ = 1 is bit for bit the kernel without a temperature; greedy picks against the CPU arg-max; tempered
  log-probs and draw frequencies against torch; edge shapes; and the slot policies (``temperature=True``: all-ones is
  the step without it, per-slot changes need no recapture, also in a mixed-version step);
* on the CPU: ``sample_heads`` (the oracle and the CPU actor's sampler) against numpy, ``set_temperature``'s
  validation, and the option through ``VecActor``, ``evaluate_vs_default_bot`` and the agent's command line.

The GPU input recipes are those of tests/test_actor_gpu.py.
"""
import numpy as np
import pytest
import torch

from dotaclient_amd import native
from dotaclient_amd.models.policy import Policy, batched_action_masks, get_config, masked_log_softmax

gpu = pytest.mark.gpu
needs_native = pytest.mark.skipif(not native.AVAILABLE, reason='native module not built')

HEADS = (('enum', 0, 3), ('x', 3, 9), ('y', 12, 9))


def _torch_logps(z, emb, handles, inv_tau=None):
    """Per-head masked log-softmax (fp32) from the packed head logits z (N,160) and unit embeddings; ``inv_tau`` (N,1):
    of the logits scaled by 1 / τ. Also returns the raw head logits."""
    U = emb.shape[1]
    valid = batched_action_masks(handles)
    lg = {k: z[:, 128 + o:128 + o + w] for k, o, w in HEADS}
    lg['target'] = torch.einsum('nd,nud->nu', z[:, :128], emb.float())
    out = {}
    for k, o, w in HEADS + (('target', 21, U),):
        x = lg[k] if inv_tau is None else lg[k] * inv_tau
        out[k] = masked_log_softmax(x, valid[:, o:o + w], dim=-1)
    return out, valid, lg


def _run_sample(C, z, emb, handles, seed=7, ctr=0, temp=None):
    N, U = handles.shape
    dev = z.device
    c = torch.tensor([ctr], dtype=torch.long, device=dev)
    idx = torch.empty(N, 4, dtype=torch.int32, device=dev)
    act = torch.empty(N, 21 + U, dtype=torch.uint8, device=dev)
    msk = torch.empty_like(act)
    logp = torch.empty(N, device=dev)
    val = torch.empty(N, device=dev)
    if temp is None:
        C.sample_actions(z, emb, handles, seed, c, idx, act, msk, logp, val)
    else:
        C.sample_actions(z, emb, handles, seed, c, idx, act, msk, logp, val, temp=temp)
    return idx.long(), act, msk, logp, val


def _first_argmax(v):
    """Lowest index of the row maximum (rows of −inf: 0)."""
    w = v.shape[1]
    cols = torch.arange(w, device=v.device).expand_as(v)
    return torch.where(v == v.amax(1, keepdim=True), cols, w).amin(1)


def _assert_record(idx, act, msk, valid, U):
    """One-hot actions of the selected heads; masks = selected heads ∧ valid (as tests/test_actor_gpu.py)."""
    N = idx.shape[0]
    dev = idx.device
    r = torch.arange(N, device=dev)
    enum, x, y, t = idx.unbind(1)
    mv, att = enum == 1, enum == 2
    A = 21 + U
    ra = torch.zeros(N, A, dtype=torch.uint8, device=dev)
    ra[r, enum] = 1
    ra[r[mv], 3 + x[mv]] = 1
    ra[r[mv], 12 + y[mv]] = 1
    ra[r[att], 21 + t[att]] = 1
    head = torch.zeros(N, A, dtype=torch.bool, device=dev)
    head[:, :3] = True
    head[:, 3:21] = mv[:, None]
    head[:, 21:] = att[:, None]
    assert torch.equal(act, ra)
    assert torch.equal(msk, (head & valid).to(torch.uint8))


@pytest.fixture(scope='module')
def consistency_inputs(gpu_ops):
    """test_sample_actions_consistency's inputs: seed 0, N = 3000, U = 40, the first 200 rows without targets."""
    torch.manual_seed(0)
    N, U = 3000, 40
    z = torch.randn(N, 160, device='cuda') * 2
    emb = (torch.randn(N, U, 128, device='cuda') * 0.2).to(torch.bfloat16)
    handles = torch.where(torch.rand(N, U, device='cuda') < 0.3, torch.randint(1, 999, (N, U), device='cuda'),
                          torch.full((N, U), -1, device='cuda'))
    handles[:200] = -1                              # rows with nothing attackable
    return z, emb, handles


# ------------------------------------------------------------------------------------------------- kernel (GPU)
@gpu
@pytest.mark.parametrize('emb_dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('handle_dtype', [torch.int64, torch.int32])
def test_temperature_one_is_the_kernel_without_it(gpu_ops, consistency_inputs, emb_dtype, handle_dtype):
    z, emb, handles = consistency_inputs
    emb, handles = emb.to(emb_dtype), handles.to(handle_dtype)
    ones = torch.ones(z.shape[0], device='cuda')
    ref = _run_sample(gpu_ops, z, emb, handles, seed=7, ctr=2)
    got = _run_sample(gpu_ops, z, emb, handles, seed=7, ctr=2, temp=ones)
    for name, a, b in zip(('idx', 'act', 'msk', 'logp', 'value'), ref, got):
        assert torch.equal(a, b), name


@gpu
def test_greedy_is_the_argmax_of_the_masked_logits(gpu_ops, consistency_inputs):
    z, emb, handles = consistency_inputs
    N, U = handles.shape
    zeros = torch.zeros(N, device='cuda')
    idx, act, msk, logp, val = _run_sample(gpu_ops, z, emb, handles, seed=7, ctr=0, temp=zeros)
    _, valid, lg = _torch_logps(z, emb, handles)
    neg = torch.full((), -torch.inf, device='cuda')
    want = {k: _first_argmax(torch.where(valid[:, o:o + w], lg[k], neg).cpu())
            for k, o, w in HEADS + (('target', 21, U),)}
    enum, x, y, t = (c.cpu() for c in idx.unbind(1))
    assert torch.equal(enum, want['enum']) and torch.equal(x, want['x']) and torch.equal(y, want['y'])
    assert not bool((enum[:200] == 2).any()), 'ATTACK selected with no valid target'
    # pointer head: fp32 reference logits; a row counts only if the reference's top-2 gap is at least 1e-4
    att = enum == 2
    top2 = torch.where(valid[:, 21:], lg['target'], neg).cpu().topk(2, dim=1).values
    clear = att & ((top2[:, 0] - top2[:, 1]) >= 1e-4)
    n_att, n_excluded = int(att.sum()), int((att & ~clear).sum())
    print(f'[greedy] ATTACK rows {n_att}, excluded for a top-2 gap < 1e-4: {n_excluded}')
    # (three iid normal enum logits: ATTACK is the largest on about a third of the 2800 rows with a target)
    assert n_att > 700 and n_excluded <= 0.01 * n_att
    assert torch.equal(t[clear], want['target'][clear])
    r = torch.arange(N, device='cuda')
    assert bool(valid[r[att.cuda()], 21 + idx[att.cuda(), 3]].all()), 'selected an invalid target'
    assert bool((logp == 0).all()) and not bool(torch.signbit(logp).any())
    torch.testing.assert_close(val, z[:, 149])
    _assert_record(idx, act, msk, valid, U)
    # no RNG: another (seed, counter) gives the same outputs
    again = _run_sample(gpu_ops, z, emb, handles, seed=1234567, ctr=9, temp=zeros)
    for name, a, b in zip(('idx', 'act', 'msk', 'logp', 'value'), (idx, act, msk, logp, val), again):
        assert torch.equal(a, b), name


@gpu
def test_greedy_ties_pick_the_lowest_index(gpu_ops, consistency_inputs):
    z, emb, handles = (t.clone() for t in consistency_inputs)
    N, U = handles.shape
    z[300, 128 + 0] = z[300, 128 + 1] = 40.0            # enum: NOOP and MOVE tie
    z[301, 128:131] = torch.tensor([0.0, 40.0, 0.0], device='cuda')
    z[301, 131 + 3] = z[301, 131 + 7] = 40.0            # x: entries 3 and 7 tie
    z[301, 140 + 8] = z[301, 140 + 2] = 40.0            # y: entries 2 and 8 tie
    # target: units 5 and 9 carry the same embedding (aligned with q: the largest logit), both valid; ATTACK forced
    z[302, 128:131] = torch.tensor([0.0, 0.0, 40.0], device='cuda')
    e = (0.5 * torch.sign(z[302, :128])).to(torch.bfloat16)
    emb[302, 5] = e
    emb[302, 9] = e
    handles[302, 5] = handles[302, 9] = 77
    idx, *_ = _run_sample(gpu_ops, z, emb, handles, temp=torch.zeros(N, device='cuda'))
    assert int(idx[300, 0]) == 0
    assert idx[301, :3].tolist() == [1, 3, 2]
    assert int(idx[302, 0]) == 2 and int(idx[302, 3]) == 5


@gpu
def test_tempered_logp_is_the_tempered_log_softmax(gpu_ops, consistency_inputs):
    z, emb, handles = consistency_inputs
    N, U = handles.shape
    r = torch.arange(N, device='cuda')
    base = _run_sample(gpu_ops, z, emb, handles, seed=7, ctr=1)
    # the four rows of a workgroup differ: τ = 0.5, 2, 1, 0
    mixed = torch.tensor([0.5, 2.0, 1.0, 0.0], device='cuda').repeat(N // 4)
    for name, tau in (('0.5', torch.full((N,), 0.5, device='cuda')), ('2', torch.full((N,), 2.0, device='cuda')),
                      ('mixed', mixed)):
        idx, act, msk, logp, val = _run_sample(gpu_ops, z, emb, handles, seed=7, ctr=1, temp=tau)
        on = tau > 0
        inv = torch.where(on, 1.0 / torch.where(on, tau, torch.ones_like(tau)), torch.ones_like(tau))
        lps, valid, _ = _torch_logps(z, emb, handles, inv_tau=inv[:, None])
        enum, x, y, t = idx.unbind(1)
        mv, att = enum == 1, enum == 2
        assert bool(valid[r[att], 21 + t[att]].all()), 'sampled an invalid target'
        assert not bool((enum[:200] == 2).any())
        ref = lps['enum'][r, enum] + mv * (lps['x'][r, x] + lps['y'][r, y]) + torch.where(att, lps['target'][r, t], 0.)
        ref = torch.where(on, ref, torch.zeros_like(ref))
        err = (logp - ref).abs()
        bound = 2e-3 * torch.clamp(inv, min=1.0) + 1e-3 * ref.abs()
        print(f'[tempered τ={name}] max |dlogp| {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
        assert bool((logp[~on] == 0).all())
        _assert_record(idx, act, msk, valid, U)
        torch.testing.assert_close(val, z[:, 149])
        if name == 'mixed':
            one = tau == 1
            assert int(one.sum()) == N // 4
            for nm, a, b in zip(('idx', 'act', 'msk', 'logp'), base, (idx, act, msk, logp)):
                assert torch.equal(a[one], b[one]), nm
            # a tempered row samples: its draws differ from the τ = 1 launch's somewhere
            assert not torch.equal(base[0][tau == 0.5], idx[tau == 0.5])


@gpu
@pytest.mark.parametrize('tau', [0.5, 2.0])
def test_tempered_draws_follow_the_tempered_softmax(gpu_ops, tau):
    """test_sample_actions_distribution's inputs (many rows sharing one set of logits) at τ ≠ 1."""
    torch.manual_seed(1)
    N, U = 40000, 40
    z1 = torch.randn(1, 160, device='cuda')
    e1 = (torch.randn(1, U, 128, device='cuda') * 0.3).to(torch.bfloat16)
    h1 = torch.full((1, U), -1, device='cuda', dtype=torch.long)
    h1[0, 1:6] = torch.arange(10, 15, device='cuda')
    z, emb, handles = z1.expand(N, -1).contiguous(), e1.expand(N, -1, -1).contiguous(), h1.expand(N, -1).contiguous()
    lps1, valid, _ = _torch_logps(z1, e1, h1)
    lpst, _, _ = _torch_logps(z1, e1, h1, inv_tau=torch.full((1, 1), 1.0 / tau, device='cuda'))
    heads = ((0, 'enum', 0, 3), (1, 'x', 3, 9), (2, 'y', 12, 9), (3, 'target', 21, U))
    ps = {}
    for col, k, o, w in heads:
        p1 = lps1[k][0].exp() * valid[0, o:o + w]
        ps[k] = lpst[k][0].exp() * valid[0, o:o + w]
        gap = float((ps[k] - p1).abs().max())
        print(f'[distribution τ={tau}] {k}: max |p_τ − p_1| = {gap:.3f}')
        assert gap > 0.05, (k, gap)                      # an untempered kernel cannot pass below
    idx, *_ = _run_sample(gpu_ops, z, emb, handles, seed=11, ctr=3, temp=torch.full((N,), tau, device='cuda'))
    for col, k, o, w in heads:
        freq = torch.bincount(idx[:, col], minlength=w).float() / N
        print(f'[distribution τ={tau}] {k}: max |freq − p_τ| = {float((freq - ps[k]).abs().max()):.4f}')
        assert (freq - ps[k]).abs().max() < 0.015, (k, freq, ps[k])


@gpu
@pytest.mark.parametrize('U', [1, 3, 64])
@pytest.mark.parametrize('no_handles', [False, True])
def test_edge_shapes(gpu_ops, U, no_handles):
    """A partial last workgroup (N = 5); only the self slot, less than one pointer iteration, lane 63 in use."""
    torch.manual_seed(4)
    N = 5
    z = torch.randn(N, 160, device='cuda') * 2
    emb = (torch.randn(N, U, 128, device='cuda') * 0.2).to(torch.bfloat16)
    handles = torch.where(torch.rand(N, U, device='cuda') < 0.6, torch.randint(1, 999, (N, U), device='cuda'),
                          torch.full((N, U), -1, device='cuda'))
    if U == 64:
        handles[1, 1:63] = -1
        handles[1, 63] = 5                               # the only target sits on lane 63
    if no_handles:
        handles[:] = -1
    valid = batched_action_masks(handles)
    for tau in (0.0, 0.5):
        idx, act, msk, logp, val = _run_sample(gpu_ops, z, emb, handles, temp=torch.full((N,), tau, device='cuda'))
        enum, x, y, t = idx.unbind(1)
        assert int(enum.min()) >= 0 and int(x.min()) >= 0 and int(y.min()) >= 0 and int(t.min()) >= 0
        assert int(enum.max()) <= 2 and int(x.max()) <= 8 and int(y.max()) <= 8 and int(t.max()) < U
        att = enum == 2
        r = torch.arange(N, device='cuda')
        assert bool(valid[r[att], 21 + t[att]].all()), 'selected an invalid target'
        assert not bool((att & ~valid[:, 21:].any(1)).any()), 'ATTACK with no valid target'
        assert bool(torch.isfinite(logp).all())
        assert bool((logp == 0).all()) if tau == 0 else bool((logp <= 0).all() and (logp < 0).any())
        torch.testing.assert_close(val, z[:, 149])
        _assert_record(idx, act, msk, valid, U)


@gpu
def test_temp_argument_is_checked(gpu_ops, consistency_inputs):
    z, emb, handles = (t[:8].contiguous() for t in consistency_inputs)
    with pytest.raises(RuntimeError):
        _run_sample(gpu_ops, z, emb, handles, temp=torch.ones(7, device='cuda'))
    with pytest.raises(RuntimeError):
        _run_sample(gpu_ops, z, emb, handles, temp=torch.ones(8, device='cuda', dtype=torch.float64))
    with pytest.raises(RuntimeError):
        _run_sample(gpu_ops, z, emb, handles, temp=torch.ones(8))


# ------------------------------------------------------------------------------------------------- policies (GPU)
def _observations(cfg, n, seed):
    rng = np.random.default_rng(seed)
    U = cfg.layout.max_units
    env = rng.standard_normal((n, 3)).astype(np.float32)
    units = rng.standard_normal((n, U, 10)).astype(np.float32)
    handles = np.where(rng.random((n, U)) < 0.5, rng.integers(1, 1000, (n, U)), -1).astype(np.int64)
    handles[:, 0] = 1
    handles[3, 1:] = -1                                  # a slot with nothing attackable
    return env, units, handles


def _policy_step(gp, obs):
    out = gp.step(*obs)
    torch.cuda.synchronize()
    return {k: np.array(v) for k, v in out.items()}


def _check_policy_temperature(make, cfg, n):
    """``make(seed, temperature)`` builds a graph-captured slot policy. All-ones ``h_temp`` is the policy without the
    option; per-slot greedy needs no recapture, is the arg-max of the step's own logits and ignores the seed."""
    plain, temp, other = make(5, False), make(5, True), make(99, True)
    assert plain.h_temp is None and bool((temp.h_temp == 1).all())
    off = temp.in_pack.off                                   # 'temp' directly after 'active', before the plan fields
    assert off['active'] < off['temp'] and all(off['temp'] < o for k, o in off.items()
                                               if k in ('rows', 'tile_set', 'slot_set'))
    assert 'temp' not in plain.in_pack.off
    for t in range(3):
        obs = _observations(cfg, n, 20 + t)
        a, b = _policy_step(plain, obs), _policy_step(temp, obs)
        _policy_step(other, obs)
        for name in ('idx', 'logp', 'value', 'actions', 'masks'):
            assert a[name].tobytes() == b[name].tobytes(), (name, t)
    graphs = (temp.graph, other.graph)
    assert graphs[0] is not None
    greedy = np.arange(n) % 2 == 0
    temp.set_temperature(0.0, rows=np.flatnonzero(greedy))
    other.set_temperature(np.where(greedy, 0.0, 1.0))
    obs = _observations(cfg, n, 30)
    a, b, c = _policy_step(plain, obs), _policy_step(temp, obs), _policy_step(other, obs)
    assert (temp.graph, other.graph) == graphs               # no recapture
    z = temp.z.cpu()
    any_target = torch.from_numpy((obs[2][:, 1:] != -1).any(1))
    enum_l = z[:, 128:131].clone()
    enum_l[~any_target, 2] = -torch.inf
    want = torch.stack([_first_argmax(enum_l), _first_argmax(z[:, 131:140]), _first_argmax(z[:, 140:149])], 1).numpy()
    assert np.array_equal(b['idx'][greedy, :3], want[greedy])
    assert not np.any(b['idx'][~any_target.numpy(), 0] == 2)
    assert np.all(b['logp'][greedy] == 0)
    for name in ('idx', 'logp', 'actions', 'masks'):
        assert b[name][greedy].tobytes() == c[name][greedy].tobytes(), name     # another seed: the same greedy play
        assert a[name][~greedy].tobytes() == b[name][~greedy].tobytes(), name   # the sampling half is untouched
    assert a['value'].tobytes() == b['value'].tobytes()
    assert not np.array_equal(b['idx'][~greedy], c['idx'][~greedy])              # (the seeds do differ)


@gpu
@pytest.mark.parametrize('preset,precision', [('lstm128', 'fp32'), ('lstm128', 'bf16'), ('lstm512', 'fp8'),
                                              ('5v5', 'fp32')])
def test_policy_temperature(gpu_ops, preset, precision):
    from dotaclient_amd.actor.batched import F32ActorPolicy, Fp8ActorPolicy, GpuActorPolicy
    cls = {'bf16': GpuActorPolicy, 'fp32': F32ActorPolicy, 'fp8': Fp8ActorPolicy}[precision]
    torch.manual_seed(3)
    cfg = get_config(preset)
    pol = Policy(cfg).cuda().eval()
    n = 32
    _check_policy_temperature(lambda seed, t: cls(pol, n, device='cuda', seed=seed, use_graph=True, temperature=t),
                              cfg, n)


@gpu
def test_mixed_version_policy_temperature(gpu_ops):
    from dotaclient_amd.actor.batched import F32ActorPolicy
    cfg = get_config('lstm128')
    pols = []
    for k in range(3):
        torch.manual_seed(40 + k)
        pols.append(Policy(cfg).cuda().eval())
    n = 32

    def make(seed, t):
        gp = F32ActorPolicy(pols[0], n, device='cuda', seed=seed, use_graph=True, n_sets=3, temperature=t)
        for k in (1, 2):
            gp.load_weights(pols[k], set=k)
        gp.h_set.numpy()[:] = np.arange(n) % 3
        return gp
    _check_policy_temperature(make, cfg, n)


# ------------------------------------------------------------------------------------------------- CPU
def test_sample_heads_against_numpy():
    """Six rows: greedy, greedy with ties, greedy without a target, τ = 0.5, τ = 2, τ = 1."""
    from dotaclient_amd.actor.runner import sample_heads
    U = 4
    rng = np.random.default_rng(0)
    lg = {'enum': rng.standard_normal((6, 3)), 'x': rng.standard_normal((6, 9)), 'y': rng.standard_normal((6, 9)),
          'target_unit': rng.standard_normal((6, U))}
    lg = {k: v.astype(np.float32) for k, v in lg.items()}
    lg['enum'][0] = [0.1, 0.2, 3.0]
    lg['enum'][1] = [2.0, 2.0, -1.0]                      # tie → 0
    lg['x'][1, [4, 6]] = 9.0                              # tie → 4
    lg['target_unit'][0] = [9.0, 1.0, 5.0, 5.0]          # slot 0 (self) is never a target; 2 and 3 tie → 2
    lg['enum'][2] = [0.0, 0.5, 7.0]                       # ATTACK largest, but nothing attackable → MOVE
    handles = np.array([[1, 2, 3, 4], [1, -1, 3, -1], [1, -1, -1, -1], [1, 2, -1, 4], [1, 2, 3, -1], [1, -1, 3, 4]])
    tvalid = handles != -1
    tvalid[:, 0] = False
    valid = np.ones((6, 21 + U), bool)
    valid[:, 2] = tvalid.any(1)
    valid[:, 21:] = tvalid
    tau = np.array([0.0, 0.0, 0.0, 0.5, 2.0, 1.0], np.float32)
    samples, actions, masks, logp = sample_heads({k: torch.from_numpy(v) for k, v in lg.items()},
                                                 torch.from_numpy(valid), U, torch.Generator().manual_seed(0),
                                                 temperature=torch.from_numpy(tau))
    s = {k: v.numpy() for k, v in samples.items()}
    assert s['enum'][:3].tolist() == [2, 0, 1]
    assert int(s['x'][1]) == 4 and int(s['target_unit'][0]) == 2
    offs = {'enum': (0, 3), 'x': (3, 9), 'y': (12, 9), 'target_unit': (21, U)}
    for i in range(3):                                     # greedy rows: the masked arg-max of every head
        for k, (o, w) in offs.items():
            m = valid[i, o:o + w]
            assert int(s[k][i]) == (int(np.argmax(np.where(m, lg[k][i], -np.inf))) if m.any() else 0), (i, k)
    assert np.all(logp.numpy()[:3] == 0)
    for i in range(3, 6):                                  # tempered rows: log-softmax of logits / τ over the mask
        want = 0.0
        e = int(s['enum'][i])
        for k, (o, w) in offs.items():
            if k == 'enum' or (k in ('x', 'y') and e == 1) or (k == 'target_unit' and e == 2):
                m = valid[i, o:o + w]
                assert m[s[k][i]]
                v = lg[k][i].astype(np.float64) / float(tau[i])
                want += v[s[k][i]] - np.log(np.exp(v[m]).sum())
        assert abs(float(logp[i]) - want) < 1e-5, (i, float(logp[i]), want)
    # the record: one-hot of the selected heads, masks = selected heads ∧ valid, whatever τ
    a, mk = actions.numpy(), masks.numpy()
    for i in range(6):
        e = int(s['enum'][i])
        ra = np.zeros(21 + U, np.uint8)
        ra[e] = 1
        head = np.zeros(21 + U, bool)
        head[:3] = True
        if e == 1:
            ra[3 + s['x'][i]] = ra[12 + s['y'][i]] = 1
            head[3:21] = True
        if e == 2:
            ra[21 + s['target_unit'][i]] = 1
            head[21:] = True
        assert np.array_equal(a[i], ra) and np.array_equal(mk[i], (head & valid[i]).astype(np.uint8)), i
    # a scalar temperature; none at all is the old sampler, draw for draw
    g = {k: torch.from_numpy(v) for k, v in lg.items()}
    s0 = sample_heads(g, torch.from_numpy(valid), U, torch.Generator().manual_seed(3))
    s1 = sample_heads(g, torch.from_numpy(valid), U, torch.Generator().manual_seed(3), temperature=1.0)
    assert all(torch.equal(s0[0][k], s1[0][k]) for k in s0[0]) and torch.allclose(s0[3], s1[3], atol=1e-6)
    s2 = sample_heads(g, torch.from_numpy(valid), U, torch.Generator().manual_seed(3), temperature=0.0)
    assert bool((s2[3] == 0).all()) and s2[0]['enum'][:3].tolist() == [2, 0, 1]


def _slot_obs(cfg, n, seed):
    rng = np.random.default_rng(seed)
    U = cfg.layout.max_units
    handles = np.where(rng.random((n, U)) < 0.5, rng.integers(1, 1000, (n, U)), -1).astype(np.int64)
    return (rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, U, 10)).astype(np.float32),
            handles)


def test_torch_slot_policy_greedy_is_seed_independent():
    from dotaclient_amd.actor.batched import TorchSlotPolicy
    cfg = get_config('lstm128')
    torch.manual_seed(0)
    pol = Policy(cfg)
    n = 8
    outs = []
    for seed in (1, 2):
        sp = TorchSlotPolicy(pol, n, seed=seed, temperature=True)
        assert bool((sp.h_temp == 1).all())
        sp.set_temperature(0.0)
        steps = []
        for t in range(3):
            env, units, handles = _slot_obs(cfg, n, 10 + t)
            sp.h_env.copy_(torch.from_numpy(env))
            sp.h_units.copy_(torch.from_numpy(units))
            sp.h_handles.copy_(torch.from_numpy(handles))
            sp.step_async()
            steps.append({k: np.array(v) for k, v in sp.wait().items()})
        outs.append(steps)
    for a, b in zip(*outs):
        assert np.array_equal(a['idx'], b['idx']) and np.array_equal(a['actions'], b['actions'])
        assert np.all(a['logp'] == 0) and np.all(b['logp'] == 0)
    # per slot: rows 0-3 sample at τ = 1 again, the rest stay greedy
    sp.set_temperature(1.0, rows=[0, 1, 2, 3])
    sp.step_async()
    o = sp.wait()
    assert np.all(o['logp'][:4] < 0) and np.all(o['logp'][4:] == 0)


def test_set_temperature_validates():
    from dotaclient_amd.actor.batched import TorchSlotPolicy, check_temperature
    from dotaclient_amd.actor.runner import PolicyRunner
    cfg = get_config('lstm128')
    pol = Policy(cfg)
    sp = TorchSlotPolicy(pol, 4, temperature=True)
    for bad in (float('nan'), -1.0, 1e-4, 1e4, float('inf'), [1.0, 1.0, 1e-4, 1.0]):
        with pytest.raises(ValueError):
            sp.set_temperature(bad)
        with pytest.raises(ValueError):
            check_temperature(bad)
    assert bool((sp.h_temp == 1).all())                    # a refused value changes nothing
    sp.set_temperature([0.0, 1e-3, 1e3, 2.0])
    assert sp.h_temp.tolist() == pytest.approx([0.0, 1e-3, 1e3, 2.0])
    with pytest.raises(RuntimeError):
        TorchSlotPolicy(pol, 4).set_temperature(0.0)      # built without the option
    with pytest.raises(ValueError):
        PolicyRunner(pol, temperature=1e-4)


def _store(cfg, versions=(0,), seed=0):
    from dotaclient_amd.actor.weights import WeightStore
    ws = WeightStore(cfg, device='cpu')
    for v in versions:
        torch.manual_seed(seed + v)
        ws.add(v, {k: t.detach().clone() for k, t in Policy(cfg).state_dict().items()})
    return ws


@needs_native
def test_vec_actor_greedy_rollouts_carry_logp_zero():
    from dotaclient_amd.actor.batched import TorchSlotPolicy
    from dotaclient_amd.actor.vec import VecActor
    from dotaclient_amd.transport.codec import decode
    ws = _store(get_config('lstm128'))
    sent = []
    va = VecActor(ws, 3, sent.append, device='cpu', seed=5, rollout_size=24, max_dota_time=15.0, hidden_stride=8,
                  threads=2, groups=1, temperature=0.0)
    assert all(isinstance(g.gp, TorchSlotPolicy) and g.gp.temperature for g in va.groups)
    while va.games_finished < 3:
        va.step()
    va.close()
    rs = [decode(b) for b in sent]
    assert rs and sum(r.length for r in rs) > 50
    assert all(np.all(np.asarray(r.logp) == 0) for r in rs)
    # the default runtime builds its policies without the option; a bad temperature is refused
    plain = VecActor(ws, 2, None, device='cpu', seed=5, max_dota_time=15.0, threads=2, groups=1)
    assert all(not g.gp.temperature and g.gp.h_temp is None for g in plain.groups)
    with pytest.raises(ValueError):
        VecActor(ws, 2, None, device='cpu', temperature=1e-4)


@needs_native
def test_greedy_evaluation_repeats():
    from dotaclient_amd.actor.validate import evaluate_vs_default_bot
    torch.manual_seed(0)
    pol = Policy(get_config('lstm128'))
    kw = dict(n_games=3, device='cpu', seed=3, max_dota_time=15.0, threads=2, temperature=0.0)
    a, b = evaluate_vs_default_bot(pol, **kw), evaluate_vs_default_bot(pol, **kw)
    assert a == b and a['games'] == 3.0


@needs_native
def test_vec_actor_mixed_league_greedy_opponents():
    """league_step='mixed', opponent_temperature=0: the slots on the snapshot sets play greedily (logp 0), the slots on
    the latest weights sample (logp < 0) — in the same policy step."""
    import random
    from dotaclient_amd.actor.league import League
    from dotaclient_amd.actor.vec import VecActor
    ws = _store(get_config('lstm128'), versions=(0, 1, 2))
    va = VecActor(ws, 4, None, device='cpu', seed=9, max_dota_time=15.0, hidden_stride=8, threads=2, groups=1,
                  latest_weights_prob=0.0, league=League(ws, mode='uniform', rng=random.Random(0)),
                  opponent_refresh=2, league_step='mixed', opponent_temperature=0.0)
    g = va.groups[0]
    seen = {'opp': 0, 'latest': 0}
    inner = g.gp.step_async

    def spy(snapshot_rows=None):
        inner(snapshot_rows=snapshot_rows)
        hset, on = g.gp.h_set.numpy(), g.gp.h_active.numpy() > 0
        temp, logp = g.gp.h_temp.numpy(), g.gp._out['logp']
        assert np.array_equal(temp, np.where(hset == 0, 1.0, 0.0).astype(np.float32))
        assert np.all(logp[on & (hset > 0)] == 0) and np.all(logp[on & (hset == 0)] < 0)
        seen['opp'] += int((on & (hset > 0)).sum())
        seen['latest'] += int((on & (hset == 0)).sum())
    g.gp.step_async = spy
    while va.games_finished < 4:
        va.step()
    va.close()
    assert seen['opp'] > 50 and seen['latest'] > 50


def test_cli_parser_takes_the_temperature_flags():
    from dotaclient_amd.cli.agent import build_parser
    ap = build_parser()
    a = ap.parse_args([])
    assert a.temperature == 1.0 and a.opponent_temperature is None
    a = ap.parse_args(['--validation', 'true', '--temperature', '0', '--opponent-temperature', '0.5'])
    assert a.validation is True and a.temperature == 0.0 and a.opponent_temperature == 0.5
    assert 'greedy' in ap.format_help()
