"""Importance-sampling weights of the prioritised mixture sampler through the loss (ops/replay.py, learner/replay.py,
learner/losses.py, ops/csrc/replay_sample.hip, ops/csrc/heads_loss.hip): the float64 oracle's identities, the weighted
torch loss against a hand-written weighted sum, the refusals of the public surface, the CPU optimizer training with
them — and on the GPU the sampler's weights against the oracle, the loss kernel's weighted outputs against its own
unweighted outputs (bitwise, power-of-two weights) and against the float64 torch loss, and the fused learner step
(beta = 0 is the step without the feature; captured = eager; priorities do not see the weights; gradients against a
float64 evaluation)."""
import copy

import numpy as np
import pytest
import torch

from dotaclient_amd.constants import LAYOUT_1V1
from dotaclient_amd.learner.losses import ppo_loss, split_heads
from dotaclient_amd.learner.replay import HbmReplay
from dotaclient_amd.ops import replay as R

ETA, ALPHA, EPS = 0.9, 0.6, 1e-3


# ---- CPU: the oracle ------------------------------------------------------------------------------------------
def _q_loop(p, idx, size, cursor, cap, recent, f):
    """q(idx) of the mixture, one draw at a time."""
    m = size if not recent else min(size, recent)
    T = float(np.sum(np.asarray(p, dtype=np.float64)))
    out = []
    for i in idx:
        win = 1.0 / m if ((cursor - 1 - int(i)) % cap) < m else 0.0
        out.append(f * win + (1.0 - f) * float(p[int(i)]) / T if T > 0 else win)
    return np.array(out)


def test_oracle_identities():
    g = torch.Generator().manual_seed(5)
    cap = 64
    p = torch.randint(1, 4096, (cap,), generator=g).double() / 1024.0
    idx = torch.randint(0, cap, (40,), generator=g)
    # beta = 0: every weight 1
    w, st = R.importance_weights_reference(p, idx, cap, 10, cap, 4, 0.5, 0.0)
    assert w.tolist() == [1.0] * 40 and st.tolist() == [40.0, 1.0, 0.0]
    # recent_frac = 1, every draw inside the window: equal probabilities 1/m, all weights 1 at any beta
    win = torch.tensor([9, 8, 7, 6, 9, 6])
    w, st = R.importance_weights_reference(p, win, cap, 10, cap, 4, 1.0, 0.7)
    assert w.tolist() == [1.0] * 6 and st.tolist() == [6.0, 1.0, 0.0]
    # recent_frac = 0, beta = 1: w = T / (size·P), normalised by the batch maximum = min P / P
    w, st = R.importance_weights_reference(p, idx, cap, 10, cap, 4, 0.0, 1.0)
    np.testing.assert_allclose(w.numpy(), (p[idx].min() / p[idx]).numpy(), rtol=4e-16, atol=0.0)
    assert float(w.max()) == 1.0 and float(st[2]) == 0.0
    # a window that wraps the ring's end (cursor 2, m = 4: slots 1, 0, 63, 62), both branches mixed
    idx2 = torch.tensor([1, 0, 63, 62, 2, 61, 30])
    w, st = R.importance_weights_reference(p, idx2, cap, 2, cap, 4, 0.5, 0.4)
    q = _q_loop(p.numpy(), idx2.tolist(), cap, 2, cap, 4, 0.5)
    raw = (cap * q) ** -0.4
    np.testing.assert_allclose(w.numpy(), raw / raw.max(), rtol=1e-15)
    assert bool((q[:4] > q[4:].max()).all())                 # the window slots carry the extra f/m
    w32 = w.numpy().astype(np.float32).astype(np.float64)
    assert st.tolist() == [float(w32.sum()), float(w32.min()), 0.0]
    # ... and with recent_frac = 1 a slot outside the window has q = 0: weight 1 before the division, counted
    w, st = R.importance_weights_reference(p, idx2, cap, 2, cap, 4, 1.0, 0.4)
    np.testing.assert_allclose(w.numpy(), [16.0 ** -0.4] * 4 + [1.0] * 3, rtol=1e-15)
    assert float(st[2]) == 3.0
    # T = 0 (nothing to prioritise): q = [in window]/m whatever recent_frac says
    z = torch.zeros(cap)
    w, st = R.importance_weights_reference(z, torch.tensor([1, 62, 5]), 8, 2, cap, 4, 0.25, 1.0)
    assert w.tolist() == [0.5, 0.5, 1.0] and float(st[2]) == 1.0      # (8·1/4)^-1 in the window; q = 0 outside it
    w, _ = R.importance_weights_reference(z, torch.tensor([1, 62]), 8, 2, cap, 4, 0.25, 1.0)
    assert w.tolist() == [1.0, 1.0]
    # size < capacity enters as N: a partly filled ring, newest window of 3 behind the cursor
    part = p.clone()
    part[40:] = 0.0
    idx3 = torch.tensor([39, 38, 37, 0, 17])
    w, _ = R.importance_weights_reference(part, idx3, 40, 40, cap, 3, 0.5, 1.0)
    q = _q_loop(part.numpy(), idx3.tolist(), 40, 40, cap, 3, 0.5)
    np.testing.assert_allclose(w.numpy(), (1.0 / q) / (1.0 / q).max(), rtol=1e-15)


# ---- CPU: the torch loss ---------------------------------------------------------------------------------------
def _loss_inputs(B, S, U, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    counts = {'enum': 3, 'x': 9, 'y': 9, 'target_unit': U}
    logits = {k: torch.randn(B, S, n, generator=g, dtype=dtype).requires_grad_() for k, n in counts.items()}
    values = torch.randn(B, S, 1, generator=g, dtype=dtype).requires_grad_()
    masks, acts = {}, {}
    for k, n in counts.items():
        m = torch.rand(B, S, n, generator=g) < 0.6
        a = torch.zeros(B, S, n)
        pick = torch.randint(0, n, (B, S), generator=g)
        chosen = torch.rand(B, S, generator=g) < (0.9 if k == 'enum' else 0.5)
        chosen[0, 1] = False                                 # a padded step: no head selects anything
        a.scatter_(-1, pick.unsqueeze(-1), chosen.float().unsqueeze(-1))
        masks[k] = (m | (a > 0)).to(torch.uint8)
        acts[k] = a.to(torch.uint8)
    adv = torch.randn(B, S, generator=g, dtype=dtype)
    ret = torch.randn(B, S, generator=g, dtype=dtype)
    lpo = -3.0 + 0.3 * torch.randn(B, S, generator=g, dtype=dtype)
    return logits, values, acts, masks, adv, ret, lpo


def _hand_weighted_loss(logits, values, acts, masks, adv, ret, lpo, clip, ent_coef, vf_coef, offpolicy, w):
    """The weighted objective written out row by row (no shared code with learner/losses.py)."""
    B, S = adv.shape
    logp = {k: torch.log_softmax(torch.where(masks[k].bool(), lg, torch.full_like(lg, -1e300)), -1)
            for k, lg in logits.items()}
    n_valid = sum(1.0 for b in range(B) for s in range(S) if sum(int(acts[k][b, s].sum()) for k in acts) > 0)
    total = 0.0
    for b in range(B):
        for s in range(S):
            if sum(int(acts[k][b, s].sum()) for k in acts) == 0:
                continue
            lp = sum((logp[k][b, s] * acts[k][b, s].double()).sum() for k in acts)
            r = torch.exp(lp - lpo[b, s])
            if offpolicy == 'tis':
                pol = r.detach().clamp(max=1.0) * adv[b, s] * (1.0 + lp - lp.detach())
            else:
                pol = torch.minimum(r * adv[b, s], r.clamp(1.0 - clip, 1.0 + clip) * adv[b, s])
            total = total + w[b] * (-pol + vf_coef * (values[b, s, 0] - ret[b, s]) ** 2) / n_valid
    for k in logits:
        n_sel = float(acts[k].sum())
        if n_sel == 0:
            continue
        for b in range(B):
            for s in range(S):
                m = masks[k][b, s].bool()
                lpk = logp[k][b, s][m]
                total = total - ent_coef * w[b] * (-(torch.exp(lpk) * lpk).sum()) / n_sel
    return total


@pytest.mark.parametrize('offpolicy', ['clip', 'tis'])
def test_ppo_loss_seq_weight_matches_hand_written_sum(offpolicy):
    B, S, U = 3, 5, 7
    logits, values, acts, masks, adv, ret, lpo = _loss_inputs(B, S, U, 11)
    w = torch.tensor([1.0, 0.37, 0.052], dtype=torch.float64)
    loss, _ = ppo_loss(logits, values, acts, masks, adv, ret, lpo, 0.2, 0.01, 0.5, offpolicy=offpolicy, seq_weight=w)
    want = _hand_weighted_loss(logits, values, acts, masks, adv, ret, lpo, 0.2, 0.01, 0.5, offpolicy, w)
    leaves = list(logits.values()) + [values]
    got_g = torch.autograd.grad(loss, leaves)
    want_g = torch.autograd.grad(want, leaves)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    for a, b in zip(got_g, want_g):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-14)
    # the weights matter: sequence 2's gradient is 0.052 of its unweighted one, the normalisers unchanged
    plain, _ = ppo_loss(logits, values, acts, masks, adv, ret, lpo, 0.2, 0.01, 0.5, offpolicy=offpolicy)
    gp = torch.autograd.grad(plain, leaves)
    torch.testing.assert_close(got_g[-1][2], 0.052 * gp[-1][2], rtol=1e-12, atol=0.0)
    torch.testing.assert_close(got_g[-1][0], gp[-1][0], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_ppo_loss_unit_weights_equal_no_weights(dtype):
    logits, values, acts, masks, adv, ret, lpo = _loss_inputs(4, 6, 9, 2, dtype)
    for off in ('clip', 'tis'):
        a, ma = ppo_loss(logits, values, acts, masks, adv, ret, lpo, 0.2, 0.01, 0.5, offpolicy=off)
        b, mb = ppo_loss(logits, values, acts, masks, adv, ret, lpo, 0.2, 0.01, 0.5, offpolicy=off,
                         seq_weight=torch.ones(4, dtype=dtype))
        assert torch.equal(a, b)
        for k in ma:
            assert torch.equal(ma[k], mb[k]), k


# ---- CPU: the public surface -----------------------------------------------------------------------------------
def test_refusals(tmp_path, capsys):
    from dotaclient_amd.cli import optimizer as cli
    from dotaclient_amd.learner.optimizer import DotaOptimizer
    from dotaclient_amd.transport.broker import InProcBroker
    from tests.test_replay_priority import _opt_cfg
    base = ['--log-dir', str(tmp_path), '--replay-capacity', '16', '--device', 'cpu']
    for argv, word in ((['--replay-priority-beta', '0.4'], 'mixture'),
                       (['--replay-priority-beta', '0.4', '--replay-sampler', 'uniform'], 'mixture'),
                       (['--replay-priority-beta', '0.4', '--replay-sampler', 'mixture', '--algo', 'vpg'], 'vpg'),
                       (['--replay-priority-beta', '1.5', '--replay-sampler', 'mixture'], '[0, 1]')):
        with pytest.raises(SystemExit) as e:
            cli.main(base + argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert '--replay-priority-beta' in err and word in err, err
    ap = cli.build_parser()
    args = ap.parse_args(base + ['--replay-sampler', 'mixture', '--replay-priority-beta', '0.4',
                                 '--replay-priority-beta-anneal', '100'])
    cli.check_args(ap, args)                                  # accepted
    assert args.replay_priority_beta == 0.4 and args.replay_priority_beta_anneal == 100
    d = ap.parse_args(base)
    assert d.replay_priority_beta == 0.0 and d.replay_priority_beta_anneal == 0       # default off
    with pytest.raises(ValueError, match='mixture'):
        DotaOptimizer(_opt_cfg(tmp_path / 'a', replay_priority_beta=0.4), InProcBroker())
    with pytest.raises(ValueError, match='ppo'):
        DotaOptimizer(_opt_cfg(tmp_path / 'b', replay_sampler='mixture', replay_priority_beta=0.4, algo='vpg',
                               advantages='gae', replay_priority_alpha=0.0), InProcBroker())
    with pytest.raises(ValueError, match='mixture'):
        HbmReplay(4, 4, LAYOUT_1V1, 32, 'cpu', priority_beta=0.5)
    with pytest.raises(ValueError, match='mixture'):
        HbmReplay(4, 4, LAYOUT_1V1, 32, 'cpu', prioritized=True, priority_beta=0.5)
    with pytest.raises(ValueError, match='priority_beta'):
        HbmReplay(4, 4, LAYOUT_1V1, 32, 'cpu', prioritized=True, sampler='mixture', priority_beta=1.5)


def test_replay_beta_state_and_annealing():
    from dotaclient_amd.learner.synthetic import make_batch
    off = HbmReplay(8, 4, LAYOUT_1V1, 32, 'cpu', prioritized=True, sampler='mixture')
    assert not off.weighted and off.beta == 0.0 and off.seq_weight(4) is None and off.set_iteration(50) == 0.0
    r = HbmReplay(8, 4, LAYOUT_1V1, 32, 'cpu', seed=3, prioritized=True, sampler='mixture', recent_frac=0.5,
                  priority_beta=0.4, priority_beta_anneal=10)
    assert r.weighted and r.sampler_state.is_weight.shape == (256,) and r.sampler_state.stats.shape == (7,)
    assert [round(r.set_iteration(i), 6) for i in (0, 5, 10, 99)] == [0.4, 0.7, 1.0, 1.0]
    const = HbmReplay(8, 4, LAYOUT_1V1, 32, 'cpu', prioritized=True, sampler='mixture', priority_beta=0.4)
    assert const.set_iteration(1000) == 0.4
    r.set_iteration(5)
    r.add(make_batch(6, 4, LAYOUT_1V1, 32, device='cpu', seed=0), version=1)
    r.update_priorities(torch.arange(6), torch.stack([torch.tensor([0.5, 1.0, 2.0, 4.0, 0.25, 1.0]), torch.zeros(6)]))
    view = r.seq_weight(8)
    assert view.data_ptr() == r.sampler_state.is_weight.data_ptr()         # a fixed address
    u = torch.empty(8, 2)
    idx = r._sample_mixture(torch.empty(8, dtype=torch.long), 2, u_out=u)
    w, ws = R.importance_weights_reference(r.priority, idx, 6, 6, 8, 2, 0.5, 0.7)
    assert torch.equal(view, w.float()) and float(view.max()) == 1.0 and float(view.min()) < 1.0
    assert r.sampler_state.stats[4:7].tolist() == ws.tolist() and r.sampler_state.is_weight[8:].eq(1).all()
    with pytest.raises(ValueError, match='256'):
        r.seq_weight(257)


def test_cpu_optimizer_trains_with_importance_weights(tmp_path):
    """The torch backend on the CPU replay: beta = 0 is the run without the options, bit for bit; beta > 0 trains,
    reports its metrics, anneals, stores the same first priorities (they do not see the weights) and moves the
    parameters elsewhere."""
    from dotaclient_amd.learner.optimizer import DotaOptimizer
    from dotaclient_amd.transport.broker import InProcBroker
    from tests.test_replay_priority import _opt_cfg, _publish

    def run(name, iterations=2, **kw):
        torch.manual_seed(0)
        br = InProcBroker()
        opt = DotaOptimizer(_opt_cfg(tmp_path / name, replay_sampler='mixture', replay_ratio=2.0, replay_recent=2,
                                     **kw), br)
        _publish(br, 8, np.random.default_rng(0))
        first = []
        real = opt.replay.update_priorities

        def upd(idx, pf):
            if not first:
                first.append((idx.clone(), pf.clone()))
            return real(idx, pf)
        opt.replay.update_priorities = upd
        opt.run(iterations=iterations)
        return opt, first[0]

    plain, f0 = run('plain')
    zero, fz = run('zero', replay_priority_beta=0.0, replay_priority_beta_anneal=0)
    assert torch.equal(plain.learner.flat.flat, zero.learner.flat.flat)
    assert torch.equal(plain.replay.priority, zero.replay.priority)
    assert not any(k in zero.last_metrics for k in ('replay/is_weight_mean', 'replay/beta'))
    opt, fw = run('beta', replay_priority_beta=0.5, replay_priority_beta_anneal=4)
    m = opt.last_metrics
    assert torch.equal(fw[0], f0[0]) and torch.equal(fw[1], f0[1])        # same first draws, same first priorities
    assert not torch.equal(opt.learner.flat.flat, plain.learner.flat.flat)
    assert m['replay/beta'] == pytest.approx(0.5 + 0.5 * 1 / 4) and opt.replay.beta == pytest.approx(0.625)
    assert 0.0 < m['replay/is_weight_min'] <= m['replay/is_weight_mean'] <= 1.0
    assert m['replay/zero_prob_draws'] == 0.0 and np.isfinite(m['loss/sum'])


# ---- GPU: the sampler ------------------------------------------------------------------------------------------
def _rings(cap, g):
    """(priority, size, cursor): priorities multiples of 2^-10 (every double sum exact in any order); a full ring with
    the cursor at 0 and slots of priority 0 inside, and a partly filled one (cursor mid-ring, the rest unfilled)."""
    q = torch.randint(1, 4096, (cap,), generator=g).float() / 1024.0
    full = torch.where(torch.rand(cap, generator=g) < 0.2, torch.zeros(cap), q)
    size = (2 * cap) // 3
    part = q.clone()
    part[size:] = 0.0
    return [(full, cap, 0), (part, size, size)]


def _ulp_diff(a, b):
    """|a − b| in units in the last place of b (float32 tensors of positive values)."""
    a, b = a.cpu().numpy().astype(np.float32), b.cpu().numpy().astype(np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(b).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize('cap', [64, 5000])
def test_sampler_weights_equal_oracle(gpu_ops, cap):
    g = torch.Generator().manual_seed(cap)
    ver = torch.randint(-1, 11, (cap,), generator=g)
    vd = ver.cuda()
    st = R.SamplerState(cap, 'cuda', seed=29)
    assert st.is_weight.shape == (256,) and st.stats.shape == (7,)
    worst, seen_below_one, c = 0.0, 0, 0
    for pri, size, cursor in _rings(cap, g):
        pd = pri.cuda()
        for B in (8, 70):
            for recent in (None, 4, 4096):
                for frac in (0.0, 0.5, 1.0):
                    c += 1
                    tag = (cap, size, cursor, B, recent, frac)
                    # the pass as it is without the feature: the yardstick of the indices and of stats[:4]
                    st.counter.fill_(c)
                    st.stats.fill_(-7.0)
                    out0 = torch.full((B,), -1, dtype=torch.long, device='cuda')
                    u = torch.full((B, 2), -1.0, device='cuda')
                    R.sample_mixture(pd, vd, st, out0, size, cursor, recent, frac, current_version=10, u_out=u)
                    want, _ = R.sample_mixture_reference(pri, size, cursor, cap, recent, frac, u, ver, 10)
                    assert torch.equal(out0.cpu(), want), tag
                    stats0 = st.stats.cpu().clone()
                    assert stats0[4:].tolist() == [-7.0] * 3, tag          # without w_out nothing behind the four
                    for beta in (0.0, 0.4, 1.0):
                        st.counter.fill_(c)
                        st.is_weight.fill_(-1.0)
                        out = torch.full((B,), -1, dtype=torch.long, device='cuda')
                        u2 = torch.full((B, 2), -1.0, device='cuda')
                        R.sample_mixture(pd, vd, st, out, size, cursor, recent, frac, current_version=10, u_out=u2,
                                         beta=beta, w_out=st.is_weight)
                        assert torch.equal(u2, u) and torch.equal(out, out0) and int(st.counter) == c + 1, (tag, beta)
                        stats = st.stats.cpu()
                        assert torch.equal(stats[:4], stats0[:4]), (tag, beta)
                        w, ws = R.importance_weights_reference(pri, out.cpu(), size, cursor, cap, recent, frac, beta)
                        got = st.is_weight.cpu()
                        assert bool((got[B:] == -1.0).all()), (tag, beta)   # the first B entries only
                        d = _ulp_diff(got[:B], w.float())
                        worst = max(worst, float(d.max()))
                        assert float(d.max()) <= 2.0, (tag, beta, d.max())
                        assert float(got[:B].max()) == 1.0 and float(got[:B].min()) > 0.0, (tag, beta)
                        assert stats[4:].numpy().astype(np.float32).tolist() == \
                            ws.numpy().astype(np.float32).tolist(), (tag, beta, stats[4:], ws)
                        if beta == 0.0:
                            assert bool((got[:B] == 1.0).all()), tag
                        else:
                            seen_below_one += int((got[:B] < 1.0).sum())
    print(f'cap {cap}: worst weight error {worst:.2f} ulp, {seen_below_one} weights below 1')
    assert seen_below_one > 0


# ---- GPU: the loss kernel --------------------------------------------------------------------------------------
LDZ = 160


def _kernel_inputs(U, S, B, emb_dtype, seed):
    from dotaclient_amd.ops.heads import batch_norms
    from tests.test_heads_loss_sparse import _rows
    N = S * B
    g = torch.Generator().manual_seed(seed)
    act, msk = _rows(N, U, g)                                 # row kinds incl. rows without any selection
    z = torch.randn(N, LDZ, generator=g).cuda()
    emb = (torch.randn(N, U, 128, generator=g) * 0.1).to(emb_dtype).cuda()
    adv = torch.randn(N, generator=g).cuda()
    ret = torch.randn(N, generator=g).cuda()
    lpo = (-4.0 + 0.5 * torch.randn(N, generator=g)).cuda()   # ratios on both sides of the clip range
    assert int((act.sum(1) == 0).sum()) > 0
    return dict(z=z, emb=emb, act=act, msk=msk, adv=adv, ret=ret, lpo=lpo, nret=torch.zeros(N, device='cuda'),
                norms=batch_norms(act, ret, False, N), N=N, U=U, S=S, B=B)


def _kernel(C, k, algo, precise, w=None):
    return C.heads_loss(k['z'], k['emb'], k['act'], k['msk'], k['adv'], k['ret'], k['lpo'], k['nret'], k['norms'],
                        algo, False, k['S'], k['B'], 0.2, 0.01, 0.5, dz_bf16=False, precise=precise, seq_weight=w)


def _bits(t):
    return t.contiguous().view(torch.int32)


KERNEL_CASES = [(U, S, B, ed, pr, algo) for U in (40, 64) for (S, B) in ((5, 3), (7, 8))
                for ed, pr in ((torch.float32, True), (torch.float32, False), (torch.bfloat16, False))
                for algo in (0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('U,S,B,emb_dtype,precise,algo', KERNEL_CASES)
def test_loss_kernel_power_of_two_weights_scale_rows_bitwise(gpu_ops, U, S, B, emb_dtype, precise, algo):
    """Weights from {1, 1/2, 1/4, 1/8}: every product by w is exact, so ∂z and ∂(pointer logits) of the weighted call
    are bitwise w[n % B] × the rows of the unweighted call (the kernel path as it was: the yardstick); logp unchanged.
    No weights and unit weights are the same outputs bit for bit."""
    k = _kernel_inputs(U, S, B, emb_dtype, 100 * U + 10 * S + B)
    dz0, dtl0, part0, lp0 = _kernel(gpu_ops, k, algo, precise)
    ones = _kernel(gpu_ops, k, algo, precise, torch.ones(B, device='cuda'))
    for a, b, name in zip((dz0, dtl0, part0, lp0), ones, ('dz', 'dtl', 'part', 'logp')):
        assert torch.equal(_bits(a), _bits(b)), name
    g = torch.Generator().manual_seed(B)
    w = (0.5 ** torch.randint(0, 4, (B,), generator=g).float()).cuda()
    w[0], w[-1] = 0.125, 1.0
    dz, dtl, part, lp = _kernel(gpu_ops, k, algo, precise, w)
    torch.cuda.synchronize()
    rw = w.repeat(S).unsqueeze(1)                             # time-major rows: row n ↔ sequence n % B
    assert torch.equal(_bits(lp), _bits(lp0))
    assert torch.equal(_bits(dz), _bits(dz0 * rw)) and torch.equal(_bits(dtl), _bits(dtl0 * rw))
    assert float(dz0.abs().max()) > 0 and not torch.equal(dz, dz0)
    # the diagnostics stay unweighted, the three loss terms do not
    sp, sp0 = part.double().sum(0), part0.double().sum(0)
    for i in (6, 7, 8, 11):
        assert float(sp[i]) == float(sp0[i]), i
    assert float(sp[1]) < float(sp0[1]) and float(sp[5]) < float(sp0[5])


@pytest.mark.gpu
@pytest.mark.parametrize('U,S,B,emb_dtype,precise,algo', KERNEL_CASES)
def test_loss_kernel_generic_weights_match_float64_loss(gpu_ops, U, S, B, emb_dtype, precise, algo):
    """Generic weights in (0, 1]: the loss terms (from `part`) and ∂z / ∂(pointer logits) against float64 autograd of
    ppo_loss(seq_weight=w) on the same logits. Bounds, those the unweighted kernel is held to against that oracle: the
    gradients 1e-5 relative (norm) at the exact instantiation (tests/test_exact_mode.py, per tensor) and 1e-4 otherwise
    (tests/test_heads_loss_sparse.py; the fp32 step's 1e-3 of tests/test_fp32_kernels.py is wider); the loss 1e-6 resp.
    1e-4 of max(1e-2, |loss|) (test_exact_mode / test_fp32_kernels)."""
    k = _kernel_inputs(U, S, B, emb_dtype, 7 + 100 * U + 10 * S + B)
    g = torch.Generator().manual_seed(3 * B)
    w = (1.0 - 0.95 * torch.rand(B, generator=g)).cuda()
    dz, dtl, part, _ = _kernel(gpu_ops, k, algo, precise, w)
    torch.cuda.synchronize()
    counts = {'enum': 3, 'x': 9, 'y': 9, 'target_unit': U}
    bm = lambda x: x.reshape(S, B, *x.shape[1:]).transpose(0, 1)      # noqa: E731  time-major rows → (B, S, …)
    zz = k['z'].double().requires_grad_()
    tl = torch.einsum('nd,nud->nu', zz[:, :128], k['emb'].double())
    logits = {'enum': bm(zz[:, 128:131]), 'x': bm(zz[:, 131:140]), 'y': bm(zz[:, 140:149]), 'target_unit': bm(tl)}
    loss, m = ppo_loss(logits, bm(zz[:, 149:150]), split_heads(bm(k['act']), counts), split_heads(bm(k['msk']), counts),
                       bm(k['adv'].double()), bm(k['ret'].double()), bm(k['lpo'].double()), 0.2, 0.01, 0.5,
                       offpolicy='tis' if algo == 2 else 'clip', seq_weight=w.double())
    rdz, rdtl = torch.autograd.grad(loss, [zz, tl])
    from tests.test_heads_loss_sparse import _rel
    nm, sp = k['norms'].double(), part.double().sum(0)
    got = {'policy_loss': -sp[0] * nm[0], 'advantage_loss': 0.5 * sp[1] * nm[0], 'entropy': (sp[2:6] * nm[2:6]).sum()}
    got_loss = got['policy_loss'] + got['advantage_loss'] - 0.01 * got['entropy']
    e_dz, e_dtl = _rel(dz[:, :150], rdz[:, :150]), _rel(dtl, rdtl)
    loss = loss.detach()
    e_l = abs(float(got_loss) - float(loss)) / max(1e-2, abs(float(loss)))
    print(f'U={U} S={S} B={B} {emb_dtype} precise={precise} algo={algo}: dz {e_dz:.2e} dtl {e_dtl:.2e} loss {e_l:.2e}')
    gtol, ltol = (1e-5, 1e-6) if precise else (1e-4, 1e-4)
    assert e_l <= ltol, (float(got_loss), float(loss))
    for name in got:
        assert abs(float(got[name]) - float(m[name])) <= 10 * ltol * max(1e-2, abs(float(m[name]))), name
    assert e_dz < gtol and e_dtl < gtol, (e_dz, e_dtl)


@pytest.mark.gpu
def test_loss_kernel_refuses_weights_it_cannot_take(gpu_ops):
    k = _kernel_inputs(40, 5, 3, torch.float32, 1)
    with pytest.raises(RuntimeError, match='VPG'):
        _kernel(gpu_ops, k, 1, False, torch.ones(3, device='cuda'))
    with pytest.raises(RuntimeError, match='per sequence'):
        _kernel(gpu_ops, k, 0, False, torch.ones(4, device='cuda'))


# ---- GPU: the whole step ---------------------------------------------------------------------------------------
N_RING, B_STEP, S_STEP = 64, 4, 32


def _setup(pol, cfg, graph_after, S=S_STEP, ring=N_RING, **rep_kw):
    from dotaclient_amd.learner.engine import Learner, LossConfig
    from tests.test_replay_priority import _vt_batch
    L = Learner(pol, LossConfig(algo='ppo', vtrace=True), device='cuda', backend='fused', dp=False,
                precision='fp32-exact')
    if graph_after:
        assert L.enable_graph(warmup=graph_after)
    rep = HbmReplay(ring, S, cfg.layout, cfg.hidden, 'cuda', seed=5, vtrace=True, prioritized=True, sampler='mixture',
                    recent_frac=0.5, priority_alpha=ALPHA, priority_eta=ETA, priority_eps=EPS, **rep_kw)
    rep.add(_vt_batch(cfg, ring, S, 9), version=3)
    return L, rep


def _steps(L, rep, n, B=B_STEP, recent=8):
    """n steps; per step the indices, the weights the step read, the loss, the priorities and parameters after it."""
    rec, real = [], rep.update_priorities

    def upd(i, pf):
        w = rep.seq_weight(i.numel())
        rec.append(dict(idx=i.clone(), w=None if w is None else w.clone()))
        return real(i, pf)
    rep.update_priorities = upd
    for _ in range(n):
        m = L.train_step_replay(rep, B, recent)
        rec[-1].update(loss=m['loss'].clone(), metrics={k: v.clone() for k, v in m.items()},
                       priority=rep.priority.clone(), flat=L.flat.flat.clone())
    torch.cuda.synchronize()
    rep.update_priorities = real
    return rec


@pytest.fixture(scope='module')
def lstm128():
    from dotaclient_amd.models.policy import Policy, get_config
    torch.manual_seed(0)
    cfg = get_config('lstm128')
    return cfg, Policy(cfg)


@pytest.fixture(scope='module')
def eager_beta(gpu_ops, lstm128):
    """Seven eager steps at beta = 0.5 (the reference of the captured run) and the first step of a beta = 0 run."""
    cfg, pol = lstm128
    L, rep = _setup(copy.deepcopy(pol), cfg, 0, priority_beta=0.5)
    rec = _steps(L, rep, 7)
    L0, rep0 = _setup(copy.deepcopy(pol), cfg, 0)
    return dict(rec=rec, first_plain=_steps(L0, rep0, 1)[0])


@pytest.mark.gpu
def test_step_beta_zero_is_the_step_without_the_feature(gpu_ops, lstm128):
    """3 eager steps + the capture + 3 replays on a replay built with beta = 0 arguments and on one built without them:
    the same parameters and priorities bit for bit, no weight buffer wired, one graph under the unweighted key."""
    cfg, pol = lstm128
    runs = []
    for kw in ({}, dict(priority_beta=0.0, priority_beta_anneal=0)):
        L, rep = _setup(copy.deepcopy(pol), cfg, 3, **kw)
        rec = _steps(L, rep, 7)
        assert L.graph is not None and len(L.graphs) == 1 and all(len(key) == 4 for key in L.graphs)
        assert not rep.weighted and all(r['w'] is None for r in rec)
        assert not any(k.startswith('replay/is_weight') for k in rec[-1]['metrics'])
        runs.append(rec)
    for a, b in zip(*runs):
        assert torch.equal(a['idx'], b['idx']) and torch.equal(a['flat'], b['flat'])
        assert torch.equal(a['priority'], b['priority']) and torch.equal(a['loss'], b['loss'])


@pytest.mark.gpu
def test_step_beta_graph_matches_eager(gpu_ops, lstm128, eager_beta):
    """beta = 0.5: the captured steps draw the eager steps' indices and weights and compute their loss and parameters;
    the weighted step has a graph key of its own."""
    cfg, pol = lstm128
    L, rep = _setup(copy.deepcopy(pol), cfg, 3, priority_beta=0.5)
    rec = _steps(L, rep, 7)
    assert L.graph is not None and len(L.graphs) == 1 and all(key[-1] == 'is_weight' for key in L.graphs)
    below = 0
    for step, (a, e) in enumerate(zip(rec, eager_beta['rec'])):
        assert torch.equal(a['idx'], e['idx']), step
        assert torch.equal(a['w'], e['w']) and float(a['w'].max()) == 1.0, step
        below += int((a['w'] < 1.0).sum())
        print(f'step {step}: |loss diff| {float((a["loss"] - e["loss"]).abs()):.3e} '
              f'|param diff| {float((a["flat"] - e["flat"]).abs().max()):.3e}')
        assert torch.equal(a['priority'], e['priority']), step
        assert torch.equal(a['loss'], e['loss']), step
        assert torch.equal(a['flat'], e['flat']), step
        for k in ('replay/is_weight_sum', 'replay/is_weight_min', 'replay/zero_prob_draws'):
            assert torch.equal(a['metrics'][k], e['metrics'][k]), (step, k)
    assert below > 0                                          # the weights were not trivially 1


@pytest.mark.gpu
def test_priorities_do_not_see_the_weights(gpu_ops, eager_beta):
    w, p = eager_beta['rec'][0], eager_beta['first_plain']
    assert torch.equal(w['idx'], p['idx'])                    # the same first draws whatever beta
    assert torch.equal(w['priority'], p['priority'])          # … and the same stored priorities
    assert bool((w['w'] < 1.0).any()) and not torch.equal(w['flat'], p['flat'])       # while the step itself differs


def _fp64_weighted_vtrace_grads(pol, batch, lc, w):
    """float64 evaluation of the weighted in-step V-trace PPO step: the eager policy in double, ops/scan.py's V-trace
    reference (double inside) on its values and log-probs, the advantage normalisation, ppo_loss(seq_weight)."""
    from dotaclient_amd.constants import EPS as ADV_EPS
    from dotaclient_amd.learner.losses import sampled_logp
    from dotaclient_amd.ops.scan import vtrace_step
    p64 = copy.deepcopy(pol).double()
    b = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    logits, values, _ = p64.forward_packed(b['env'], b['units'], (b['h0'].unsqueeze(0), b['c0'].unsqueeze(0)))
    counts = p64.layout.action_counts()
    acts, msks = split_heads(b['actions'], counts), split_heads(b['masks'], counts)
    B, S = b['env'].shape[:2]
    tm = lambda x: x.detach().transpose(0, 1).reshape(B * S, *x.shape[2:]).cpu()      # noqa: E731
    with torch.no_grad():
        lp = sampled_logp(logits, acts, msks)
        adv, ret, _ = vtrace_step(tm(values.squeeze(-1)), tm(lp), tm(b['logp_old']), tm(b['vt']), B, S, lc.gamma,
                                  lc.gae_lambda, lc.vtrace_rho_bar, lc.vtrace_c_bar)
        back = lambda x: x.double().reshape(S, B).t().contiguous().cuda()             # noqa: E731
        adv, ret = back(adv), back(ret)
        v = b['vt'][..., 2]
        n = v.sum().clamp_min(1.0)
        mu = (adv * v).sum() / n
        sd = (((adv - mu) ** 2 * v).sum() / n).sqrt()
        adv = ((adv - mu) / (sd + ADV_EPS)) * v
    loss, _ = ppo_loss(logits, values, acts, msks, adv, ret, b['logp_old'], lc.clip_eps, lc.entropy_coef, lc.vf_coef,
                       seq_weight=w.double())
    names = [n for n, _ in p64.named_parameters()]
    return float(loss), dict(zip(names, torch.autograd.grad(loss, list(p64.parameters()), allow_unused=True)))


@pytest.mark.gpu
def test_weighted_step_gradients_match_float64(gpu_ops, lstm128):
    """Every gradient tensor of one weighted fused step (fp32-exact, in-step V-trace) within the bound of
    tests/test_exact_mode.py of the float64 evaluation: 1e-5 relative, or 1.5× the error of the torch-fp32 evaluation
    of the same weighted step where that is larger."""
    from dotaclient_amd.learner.engine import Learner, LossConfig
    from tests.test_fp32_kernels import _rel
    from tests.test_replay_priority import _vt_batch
    cfg, pol = lstm128
    lc = LossConfig(algo='ppo', vtrace=True)
    fused = Learner(copy.deepcopy(pol), lc, device='cuda', backend='fused', dp=False, precision='fp32-exact')
    oracle = Learner(copy.deepcopy(pol), lc, device='cuda', backend='torch', dp=False, precision='fp32')
    batch = _vt_batch(cfg, B_STEP, S_STEP, 3)
    w = torch.tensor([1.0, 0.61, 0.33, 0.08], device='cuda')
    fused.model.seq_weight = oracle._seq_weight = w
    out = []
    for L in (fused, oracle):
        L.dp.zero_grad()
        loss, _ = L.loss(batch)
        loss.backward()
        out.append((float(loss.detach()), {n: p.grad.detach().clone() if p.grad is not None else None
                                           for n, p in zip(L.flat.names, L.flat.params)}))
    torch.cuda.synchronize()
    fused.model.check_error()
    (lf, gf), (lo, go) = out
    l64, g64 = _fp64_weighted_vtrace_grads(copy.deepcopy(pol).cuda(), batch, lc, w)
    fused.model.seq_weight = None
    fused.dp.zero_grad()
    lu, _ = fused.loss(batch)
    assert abs(float(lu) - lf) > 1e-4                         # the weights reached the loss
    rows = sorted(((_rel(gf[n], g64[n]), _rel(go[n], g64[n]), n) for n in g64
                   if g64[n] is not None and g64[n].norm() > 0), reverse=True)
    print('weighted step: worst (fused vs fp64, torch-fp32 vs fp64):', rows[:5], 'loss', lf, lo, l64)
    assert abs(lf - l64) <= 1e-6 * max(1e-2, abs(l64)), (lf, l64)
    bad = [r for r in rows if r[0] >= max(1e-5, 1.5 * r[1])]
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_5v5_weighted_step_graph_matches_eager(gpu_ops):
    """The 5v5 entity-attention policy (U = 64) through the fused step with weights, B = 2, S = 8: captured = eager."""
    from dotaclient_amd.models.policy import Policy, get_config
    torch.manual_seed(0)
    cfg = get_config('5v5')
    pol = Policy(cfg)
    runs = []
    for graph_after in (0, 1):
        L, rep = _setup(copy.deepcopy(pol), cfg, graph_after, S=8, ring=6, priority_beta=0.5)
        runs.append(_steps(L, rep, 3, B=2, recent=3))
        assert (L.graph is not None) == bool(graph_after)
    for step, (e, a) in enumerate(zip(*runs)):
        assert torch.equal(a['idx'], e['idx']) and torch.equal(a['w'], e['w']), step
        assert torch.equal(a['priority'], e['priority']) and torch.equal(a['loss'], e['loss']), step
        assert torch.equal(a['flat'], e['flat']), step
    assert any(bool((r['w'] < 1.0).any()) for r in runs[0])
