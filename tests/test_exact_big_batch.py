"""fp32-exact beyond 32 sequences per step and GPU: the exact plan of the team recurrence (ops/csrc/lstm_team.h
``plan_exact``: exact VALU chains of 1 / 2 / 4 / 8 rows at every batch size, queued behind the 8 running ones beyond
8 × 8 sequences, at most 32 chains) from the launch plan up to ``DotaOptimizer``.

CPU: ``ops.lstm.team_plan`` against today's formula and its own invariants. GPU, kernel level: the plan the extension
reports; queued chains bit for bit the same rows launched alone; float64 with the merged 4-row kernel's own error as the
yardstick; relaunches and graph replays; refused arguments. GPU, whole step: the fused step against float64 at B = 40
and 64 (refused with a ValueError before this plan existed), packing at B = 40, and ``DotaOptimizer`` staying at
fp32-exact at batch 40."""
import copy

import pytest
import torch

from dotaclient_amd.ops.lstm import EXACT_MAX_BATCH, EXACT_MAX_CHAINS, EXACT_ROWS, team_plan

gpu = pytest.mark.gpu
RMAX = EXACT_ROWS[-1]
BIG_ROWS = [r for r in (4, 8) if r in EXACT_ROWS]        # the row forms that queue


# ------------------------------------------------------------------------------------------------ CPU: the plan
def _old_plan(B, f32):
    """plan() of lstm_team.h as it stood before the exact plan."""
    nch = min(B, 8) if B <= 8 * 32 else (B + 31) // 32
    if f32 and (B + nch - 1) // nch > 16:
        nch = (B + 15) // 16
    return nch, (B + nch - 1) // nch


def _covered(B, nch, Bc):
    rows = []
    for c in range(nch):
        rows += list(range(c * Bc, min((c + 1) * Bc, B)))
    return rows


def test_team_plan_without_exact_is_todays_formula():
    for B in range(1, 301):
        for f32 in (False, True):
            assert team_plan(B, f32, False) == _old_plan(B, f32), (B, f32)


def test_team_plan_exact_keeps_todays_plan_up_to_32():
    for B in range(1, 33):
        assert team_plan(B, True, True) == _old_plan(B, True), B


def test_team_plan_exact_covers_every_row_once():
    assert EXACT_MAX_BATCH == EXACT_MAX_CHAINS * RMAX
    for B in range(1, 301):
        if B > EXACT_MAX_BATCH:
            with pytest.raises(ValueError):
                team_plan(B, True, True)
            continue
        nch, Bc = team_plan(B, True, True)
        assert 1 <= Bc <= RMAX and 1 <= nch <= EXACT_MAX_CHAINS, (B, nch, Bc)
        assert _covered(B, nch, Bc) == list(range(B)), (B, nch, Bc)
        if B > 8 * RMAX:
            assert (nch, Bc) == ((B + RMAX - 1) // RMAX, RMAX), (B, nch, Bc)
        else:
            assert nch == min(B, 8), (B, nch)             # the 8 teams first
        for r in EXACT_ROWS:
            if (B + r - 1) // r <= EXACT_MAX_CHAINS:
                assert team_plan(B, True, True, rows=r) == ((B + r - 1) // r, r), (B, r)
                assert _covered(B, (B + r - 1) // r, r) == list(range(B))
            else:
                with pytest.raises(ValueError):
                    team_plan(B, True, True, rows=r)


@pytest.mark.parametrize('rows', [-1, 3, 5, 6, 7, 16] + [r for r in (8,) if r not in EXACT_ROWS])
def test_team_plan_refuses_bad_rows(rows):
    with pytest.raises(ValueError):
        team_plan(8, True, True, rows=rows)


def test_team_plan_refuses_rows_without_exact_and_exact_without_fp32():
    with pytest.raises(ValueError):
        team_plan(8, True, False, rows=4)
    with pytest.raises(ValueError):
        team_plan(8, False, True)
    with pytest.raises(ValueError):
        team_plan(0, True, True)


# ------------------------------------------------------------------------------------ GPU: the recurrence kernels
_FWD = ('hs', 'cs', 'gates', 'hn', 'cn')
_PER_ROW = _FWD + ('dg', 'dh0', 'dc0')
_OUT = _PER_ROW + ('db',)
_BATCH_DIM = {'hs': 1, 'cs': 1, 'gates': 1, 'dg': 1, 'hn': 0, 'cn': 0, 'dh0': 0, 'dc0': 0}


def _case(B, S, H):
    """Inputs (non-zero h0 / c0) and episode starts at t = 0, t = S - 1 and on two consecutive steps, as
    tests/test_team_bwd_handoff.py places them."""
    from test_team_bwd_handoff import _starts
    from test_team_wave_gather import _inputs
    return _inputs(B, S, H), _starts(B, S)


def _launch(C, d, reset, exact=True, rows=0, lo=None, hi=None):
    """One time-major forward + backward pair of the sequences [lo, hi) (default: all of them)."""
    from dotaclient_amd.ops.lstm import team_bwd, team_fwd
    if lo is None:
        sel = lambda x, dim: x                                        # noqa: E731
    else:
        sel = lambda x, dim: x.narrow(dim, lo, hi - lo).contiguous()  # noqa: E731
    h0, c0, rs = sel(d['h0'], 0), sel(d['c0'], 0), sel(reset, 1)
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    hs, _, cs, gates, hn, cn = team_fwd(C, sel(d['xp'], 1), d['whh'], h0, c0, err, False, exact=exact, rows=rows,
                                        time_major=True, bias4=d['bias'], reset=rs)
    dg, dh0, dc0, db = team_bwd(C, sel(d['dh'], 1), gates, cs, c0, None, None, d['whh'], err, exact=exact, rows=rows,
                                time_major=True, want_dbias=True, reset=rs)
    return {'hs': hs, 'cs': cs, 'gates': gates, 'hn': hn, 'cn': cn, 'dg': dg, 'dh0': dh0, 'dc0': dc0, 'db': db,
            'err': err}


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@gpu
@pytest.mark.parametrize('B', [8, 32, 33, 40, 64, 72])
def test_extension_reports_the_python_plan(gpu_ops, B):
    C = gpu_ops
    nch, Bc = team_plan(B, True, True)
    assert C.lstm_team_chains(B, True, True, 0) == nch
    assert C.lstm_team_chains(B, True, False, 0) == team_plan(B, True, False)[0]
    for H in (128, 512):
        assert C.lstm_team_workspace(B, H, False, True, True, 0) == 8 * 2 * Bc * H * 8
        assert C.lstm_team_workspace(B, H, True, True, True, 0) == 8 * 2 * Bc * H * 2 * 16
    for r in EXACT_ROWS:
        if (B + r - 1) // r <= EXACT_MAX_CHAINS:
            assert C.lstm_team_chains(B, True, True, r) == (B + r - 1) // r
            assert C.lstm_team_workspace(B, 256, False, True, True, r) == 8 * 2 * r * 256 * 8


@gpu
@pytest.mark.parametrize('r', BIG_ROWS)
@pytest.mark.parametrize('shape', ['one_more_chain_than_teams', 'second_round', 'partial_last_chain'])
def test_queued_chains_are_row_independent_bitwise(gpu_ops, r, shape):
    """9 chains on 8 teams: (8r + 1, 24, 128) — one more chain than teams, its last of one row; (9r, 16, 512) — a full
    ninth chain; (8r + r/2 + 1, 20, 256) — a partial last chain with more live rows than half a chain. Every chain's
    rows against the same rows launched alone at the same rows per chain: one instantiation, so bit for bit."""
    B, S, H = {'one_more_chain_than_teams': (8 * r + 1, 24, 128), 'second_round': (9 * r, 16, 512),
               'partial_last_chain': (8 * r + r // 2 + 1, 20, 256)}[shape]
    d, reset = _case(B, S, H)
    full = _launch(gpu_ops, d, reset, rows=r)
    nch, Bc = team_plan(B, True, True, rows=r)
    assert (nch, Bc) == (9, r)
    for c in range(nch):
        lo, hi = c * r, min((c + 1) * r, B)
        one = _launch(gpu_ops, d, reset, rows=r, lo=lo, hi=hi)
        torch.cuda.synchronize()
        assert int(one['err'].item()) == 0
        for k in _PER_ROW:
            assert torch.equal(full[k].narrow(_BATCH_DIM[k], lo, hi - lo), one[k]), (k, c)
    assert int(full['err'].item()) == 0


@gpu
@pytest.mark.parametrize('shape', [(40, 24, 512), (64, 32, 128)])
def test_exact_plan_matches_float64_like_the_four_row_kernel(gpu_ops, shape):
    """Every output within max(1e-6, 1.5 × e4) of the float64 recurrence, e4 being the error of the path that existed
    before — rows 0-31 in one launch of 32 (four rows per chain) and the rest in a second one — on the same data: the
    forms differ in nothing per row and only in the grouping of the bias-gradient partial sums."""
    from test_team_wave_gather import _lstm_ref
    B, S, H = shape
    d, reset = _case(B, S, H)
    X = d['xp'].double().requires_grad_(True)
    H0 = d['h0'].double().requires_grad_(True)
    C0 = d['c0'].double().requires_grad_(True)
    hr, cr, gr = _lstm_ref(X, d['bias'].double(), d['whh'].double(), H0, C0, reset.double())
    gx, gh0, gc0 = torch.autograd.grad((hr * d['dh'].double()).sum(), [X, H0, C0])
    ref = {'hs': hr.detach(), 'cs': cr.detach(), 'gates': gr.detach(), 'hn': hr[-1].detach(), 'cn': cr[-1].detach(),
           'dg': gx, 'dh0': gh0, 'dc0': gc0, 'db': gx.sum((0, 1)).t().reshape(-1)}
    new = _launch(gpu_ops, d, reset)
    a = _launch(gpu_ops, d, reset, exact=False, lo=0, hi=32)
    b = _launch(gpu_ops, d, reset, exact=False, lo=32, hi=B)
    torch.cuda.synchronize()
    for o in (new, a, b):
        assert int(o['err'].item()) == 0
    old = {k: torch.cat([a[k], b[k]], _BATCH_DIM[k]) for k in _PER_ROW}
    old['db'] = a['db'] + b['db']
    bad = []
    for k in _OUT:
        e, e4 = _rel(new[k], ref[k]), _rel(old[k], ref[k])
        print(f'{shape} {k}: exact plan {e:.3e}, 4-row launches {e4:.3e}')
        if not e <= max(1e-6, 1.5 * e4):
            bad.append((k, e, e4))
    assert not bad, bad


@gpu
def test_exact_plan_relaunches_and_graph_replays_are_bitwise_equal(gpu_ops):
    d, reset = _case(40, 16, 128)
    runs = [_launch(gpu_ops, d, reset) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs:
        assert int(r['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(r[k], runs[0][k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # eager run on the capture stream: its control block, allocator
        _launch(gpu_ops, d, reset)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
        cap = _launch(gpu_ops, d, reset)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(cap['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(cap[k], runs[0][k]), k
        for k in _OUT:                          # the next replay has to write them again
            cap[k].zero_()


@gpu
def test_refused_arguments_launch_nothing(gpu_ops):
    d, reset = _case(8, 12, 128)
    good = _launch(gpu_ops, d, reset)
    torch.cuda.synchronize()
    bad_rows = [3] + [r for r in (8,) if r not in EXACT_ROWS]
    for rows in bad_rows:
        with pytest.raises(RuntimeError):
            _launch(gpu_ops, d, reset, rows=rows)
    with pytest.raises(RuntimeError):
        _launch(gpu_ops, d, reset, exact=False, rows=RMAX)
    Bbig = EXACT_MAX_BATCH + 1
    big = {'xp': torch.zeros(2, Bbig, 128, 4, device='cuda'), 'bias': d['bias'], 'whh': d['whh'],
           'h0': torch.zeros(Bbig, 128, device='cuda'), 'c0': torch.zeros(Bbig, 128, device='cuda'),
           'dh': torch.zeros(2, Bbig, 128, device='cuda')}
    with pytest.raises(RuntimeError):
        _launch(gpu_ops, big, torch.zeros(2, Bbig, dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError):
        gpu_ops.lstm_team_chains(Bbig, True, True, 0)
    again = _launch(gpu_ops, d, reset)
    torch.cuda.synchronize()
    assert int(again['err'].item()) == 0 and int(good['err'].item()) == 0
    for k in _OUT:
        assert torch.equal(again[k], good[k]), k


# --------------------------------------------------------------------------------------------- GPU: the whole step
@gpu
@pytest.mark.parametrize('preset,B,S', [('lstm128', 40, 48), ('lstm512', 64, 32)])
def test_exact_fused_step_beyond_32_sequences_matches_fp64(gpu_ops, preset, B, S):
    """The assertions of test_exact_fused_step_deploy_shape_matches_fp64 at 40 and 64 sequences: 5 rows per chain on 8
    teams, and 8 full chains."""
    from tests.test_fp32_kernels import _rel as rel, _step_grads
    (lf, _, gf), (lo, _, go), (l64, g64) = _step_grads('fp32-exact', preset, 'ppo', B, S, fp64=True)
    rows = sorted(((rel(gf[n], g64[n]), rel(go[n], g64[n]), n) for n in g64
                   if g64[n] is not None and g64[n].norm() > 0), reverse=True)
    print(f'fp32-exact {preset} B={B} S={S}: worst (fused vs fp64, torch-fp32 vs fp64):', rows[:5], 'loss', lf, lo, l64)
    assert abs(lf - l64) <= 1e-6 * max(1e-2, abs(l64)), (lf, l64)
    bad = [r for r in rows if r[0] >= max(1e-5, 1.5 * r[1])]
    assert not bad, bad[:5]


def _packed_and_padded(cfg, n, S, device):
    """Padded: 2n sequences [A_i | pad], [B_i | pad]; packed: n sequences [A_i | B_i | pad] with a reset at |A_i|."""
    from dotaclient_amd.learner.synthetic import make_batch
    src = make_batch(2 * n, S, cfg.layout, cfg.hidden, device='cpu', seed=3, pad_frac=0.0)
    la = [3 + (5 * i) % (S // 2 - 3) for i in range(n)]
    lb = [2 + (7 * i) % (S // 2 - 2) for i in range(n)]
    pad = {k: v.clone() for k, v in src.items()}
    for k, v in pad.items():
        if v.dim() >= 2 and v.shape[1] == S:
            for i in range(n):
                v[2 * i, la[i]:] = 0
                v[2 * i + 1, lb[i]:] = 0
    pad['h0'].zero_()
    pad['c0'].zero_()
    packed = {}
    for k, v in pad.items():
        if v.dim() >= 2 and v.shape[1] == S:
            p = torch.zeros_like(v[:n])
            for i in range(n):
                p[i, :la[i]] = v[2 * i, :la[i]]
                p[i, la[i]:la[i] + lb[i]] = v[2 * i + 1, :lb[i]]
            packed[k] = p
        else:
            packed[k] = v[:n].clone()
    rst = torch.zeros(n, S, dtype=torch.uint8)
    for i in range(n):
        rst[i, la[i]] = 1
    packed['reset'] = rst
    mv = lambda d: {k: v.to(device) for k, v in d.items()}     # noqa: E731
    return mv(pad), mv(packed)


@gpu
def test_packed_step_of_40_sequences_matches_padded(gpu_ops):
    """tests/test_packing.py's GPU case at 40 packed sequences (5 rows per chain) against their 80 padded ones (10
    queued chains of 8), at its fp32-exact tolerance."""
    from dotaclient_amd.learner.engine import Learner, LossConfig
    from dotaclient_amd.models.policy import Policy, get_config
    torch.manual_seed(0)
    cfg = get_config('lstm128')
    pol = Policy(cfg)
    pad, packed = _packed_and_padded(cfg, 40, 32, 'cuda')

    def run(batch):
        p = copy.deepcopy(pol)
        lrn = Learner(p, LossConfig(algo='ppo', vf_coef=0.5, entropy_coef=0.01), device='cuda', backend='fused',
                      dp=False, precision='fp32-exact')
        lrn.dp.zero_grad()
        loss, _ = lrn.loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        lrn.model.check_error()
        return float(loss), {n: q.grad.detach().clone() for n, q in p.named_parameters() if q.grad is not None}
    l_pad, g_pad = run(pad)
    l_pack, g_pack = run(packed)
    assert abs(l_pad - l_pack) <= 1e-5 * max(1.0, abs(l_pad)), (l_pad, l_pack)
    for n, g in g_pad.items():
        rel = ((g_pack[n] - g).norm() / g.norm().clamp_min(1e-12)).item()
        assert rel < 1e-5, (n, rel)


@gpu
def test_optimizer_trains_batch_40_at_fp32_exact(gpu_ops, tmp_path):
    """``DotaOptimizer`` at batch 40 stays at fp32-exact (it used to retrain at fp32 with bf16x3 operands), its error
    word stays clear, and the captured step trains bit for bit like the eager one."""
    from test_learner_async import _rollout
    from dotaclient_amd.learner.optimizer import DotaOptimizer, OptimizerConfig
    from dotaclient_amd.transport.broker import InProcBroker
    from dotaclient_amd.transport.codec import encode
    outs = []
    for graph in (False, True):
        br = InProcBroker()
        for i in range(96):
            br.publish_experience(encode(_rollout(i, T=32)))
        cfg = OptimizerConfig(log_dir=str(tmp_path / f'g{int(graph)}'), model='lstm128', epochs=1, seq_per_epoch=40,
                              batch_size=40, seq_len=32, device='cuda', xp_timeout=30, precision='fp32-exact',
                              graph=graph)
        opt = DotaOptimizer(cfg, br)
        opt.run(iterations=2)
        torch.cuda.synchronize()
        assert opt.learner.precision == 'fp32-exact'
        assert opt.learner.backend == 'fused'
        opt.learner.model.check_error()
        outs.append(opt.learner.flat.flat.detach().cpu().clone())
    assert torch.equal(outs[0], outs[1])
