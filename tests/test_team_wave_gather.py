"""The exact-fp32 (V1 / V2) team recurrences with the backward's wave-private gather: every wave of a workgroup
polls only the chunks of its own K part of ∂G_{t+1} and no workgroup barrier stands between that gather and the
partial product (ops/csrc/lstm_team_bwd.hip). Checked here: forward and backward against a float64 recurrence at the
shapes where the first step (no gather), the first gather and the final ∂h0 iteration, waves without units, uneven
chains and the 2- and 4-row forms can go wrong; episode-start flags; row b of a B-row launch bitwise equal to that
row launched alone (a wave that read bytes it did not fetch itself shows up here); back-to-back and hipGraph-replayed
launches bitwise equal (control block, tags and LDS images survive relaunches); the error word stays 0. The
``precise`` (libm activation) forms of the one-row chains at each H go through the same float64 check, and ``precise``
with more rows per chain, for which no kernel exists, is refused before anything runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, S, H): S = 1 / 2 — the no-gather first step, the first gather, the final ∂h0 iteration; H = 128 / 256 — waves
# that own no units, other K parts; B = 9 — uneven two-row chains; B = 16 / 32 — two / four rows per chain
SHAPES = [(1, 1, 512), (1, 2, 512), (8, 33, 512), (3, 40, 128), (5, 17, 256), (9, 20, 128), (16, 12, 512),
          (32, 9, 512)]
# precise: one-row chains at each H (H = 512: the backward's eight-wave form)
PRECISE_SHAPES = [(3, 5, 128), (2, 5, 256), (8, 5, 512)]
CASES = ([(s, True, False) for s in SHAPES] + [((8, 33, 512), False, False), ((3, 40, 128), False, False)] +
         [(s, True, True) for s in PRECISE_SHAPES])
CASE_IDS = [f'shape{i}-{tm}' + ('-precise' if p else '') for i, (_, tm, p) in enumerate(CASES)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _g(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _lstm_ref(xp4, bias4, whh, h0, c0, reset=None):
    """float64 recurrence on unit-major gates: xp4 (S,B,H,4) time-major, whh (4H,H) gate-major rows; reset (S,B):
    1 where an episode starts (h and c are zero before that step)."""
    S, B, H, _ = xp4.shape
    h, c = h0, c0
    hs, cs, gs = [], [], []
    for t in range(S):
        if reset is not None:
            keep = (1.0 - reset[t])[:, None]
            h, c = h * keep, c * keep
        pre = xp4[t] + bias4.view(H, 4) + (h @ whh.t()).view(B, 4, H).transpose(1, 2)
        i, f, gg, o = pre.unbind(-1)
        i, f, o, gg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.stack([i, f, gg, o], -1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def _inputs(B, S, H):
    """Time-major inputs from a fixed generator (fp32 W_hh: the exact VALU forms run for chains of ≤ 4 rows)."""
    g = _g(B * 100 + S)
    d = {'xp': torch.randn(S, B, H, 4, device='cuda', generator=g) * 0.5,
         'bias': torch.randn(4 * H, device='cuda', generator=g) * 0.3,
         'whh': torch.randn(4 * H, H, device='cuda', generator=g) * (1.0 / H ** 0.5),
         'h0': torch.randn(B, H, device='cuda', generator=g) * 0.3,
         'c0': torch.randn(B, H, device='cuda', generator=g) * 0.3,
         'dh': torch.randn(S, B, H, device='cuda', generator=g)}
    return d


def _starts(B, S):
    """(S, B) u8 episode-start flags: t = 0, t = S - 1, mid-sequence, all three in one row, then scattered."""
    r = torch.zeros(S, B, dtype=torch.uint8)
    r[0, 0] = 1
    r[S - 1, 1 % B] = 1
    r[S // 2, 2 % B] = 1
    for t in (0, S // 2, S - 1):
        r[t, 3 % B] = 1
    for b in range(4, B):
        r[(5 * b + 3) % S, b] = 1
    return r.cuda()


def _launch(C, d, time_major=True, reset=None, rows=None, precise=False):
    """One forward + backward pair; returns the outputs in time-major order (views for batch-major launches)."""
    from dotaclient_amd.ops.lstm import team_bwd, team_fwd
    sel = (lambda x, dim: x) if rows is None else (lambda x, dim: x.narrow(dim, rows, 1).contiguous())
    lay = (lambda x: x) if time_major else (lambda x: x.transpose(0, 1).contiguous())
    xp, dh = lay(sel(d['xp'], 1)), lay(sel(d['dh'], 1))
    h0, c0 = sel(d['h0'], 0), sel(d['c0'], 0)
    rs = None if reset is None else lay(sel(reset, 1))
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    hs, _, cs, gates, hn, cn = team_fwd(C, xp, d['whh'], h0, c0, err, False, time_major=time_major, bias4=d['bias'],
                                        reset=rs, precise=precise)
    dg, dh0, dc0, db = team_bwd(C, dh, gates, cs, c0, None, None, d['whh'], err, time_major=time_major,
                                want_dbias=True, reset=rs, precise=precise)
    tm = (lambda x: x) if time_major else (lambda x: x.transpose(0, 1))
    return {'hs': tm(hs), 'cs': tm(cs), 'gates': tm(gates), 'hn': hn, 'cn': cn, 'dg': tm(dg), 'dh0': dh0, 'dc0': dc0,
            'db': db, 'err': err}


_REF = {}


def _reference(B, S, H, with_reset):
    """float64 forward and gradients of one shape, computed once and shared (read-only) by the tests that need it."""
    key = (B, S, H, with_reset)
    if key not in _REF:
        d = _inputs(B, S, H)
        reset = _starts(B, S) if with_reset else None
        X = d['xp'].double().requires_grad_(True)
        H0 = d['h0'].double().requires_grad_(True)
        C0 = d['c0'].double().requires_grad_(True)
        hr, cr, gr = _lstm_ref(X, d['bias'].double(), d['whh'].double(), H0, C0,
                               None if reset is None else reset.double())
        gx, gh0, gc0 = torch.autograd.grad((hr * d['dh'].double()).sum(), [X, H0, C0])
        _REF[key] = (d, reset, {'hs': hr.detach(), 'cs': cr.detach(), 'gates': gr.detach(), 'hn': hr[-1].detach(),
                                'cn': cr[-1].detach(), 'dg': gx, 'dh0': gh0, 'dc0': gc0,
                                'db': gx.sum((0, 1)).t().reshape(-1)})     # gate-major, PyTorch's b_ih / b_hh order
    return _REF[key]


def _check(out, ref):
    torch.cuda.synchronize()
    assert int(out['err'].item()) == 0
    for k in ('hs', 'cs', 'gates', 'hn', 'cn'):
        assert _rel(out[k], ref[k]) < 2e-5, (k, _rel(out[k], ref[k]))
    for k in ('dg', 'dh0', 'dc0', 'db'):
        assert _rel(out[k], ref[k]) < 1e-4, (k, _rel(out[k], ref[k]))


@pytest.mark.parametrize('shape,time_major,precise', CASES, ids=CASE_IDS)
def test_wave_gather_matches_float64(gpu_ops, shape, time_major, precise):
    d, _, ref = _reference(*shape, False)
    _check(_launch(gpu_ops, d, time_major=time_major, precise=precise), ref)


def test_precise_needs_one_row_chains(gpu_ops):
    """fp32 weights, B = 16: two rows per chain. There is no libm-activation kernel for them, so forward and backward
    raise, and nothing ran that could have set the error word."""
    from dotaclient_amd.ops.lstm import team_bwd, team_fwd
    d = _inputs(16, 3, 512)
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError):
        team_fwd(gpu_ops, d['xp'], d['whh'], d['h0'], d['c0'], err, False, time_major=True, bias4=d['bias'],
                 precise=True)
    hs, _, cs, gates, _, _ = team_fwd(gpu_ops, d['xp'], d['whh'], d['h0'], d['c0'], err, False, time_major=True,
                                      bias4=d['bias'])
    with pytest.raises(RuntimeError):
        team_bwd(gpu_ops, d['dh'], gates, cs, d['c0'], None, None, d['whh'], err, time_major=True, want_dbias=True,
                 precise=True)
    torch.cuda.synchronize()
    assert int(err.item()) == 0


@pytest.mark.parametrize('shape', [(8, 33, 512), (9, 20, 128)])
def test_wave_gather_episode_starts(gpu_ops, shape):
    d, reset, ref = _reference(*shape, True)
    _check(_launch(gpu_ops, d, reset=reset), ref)


@pytest.mark.parametrize('shape', [(8, 33, 512), (3, 40, 128)])
def test_wave_gather_rows_bitwise_independent(gpu_ops, shape):
    """Both launches run the one-row instantiation: row b among B rows must equal row b alone, bit for bit."""
    B = shape[0]
    d = _reference(*shape, False)[0]
    full = _launch(gpu_ops, d)
    for b in range(B):
        one = _launch(gpu_ops, d, rows=b)
        torch.cuda.synchronize()
        assert int(one['err'].item()) == 0
        for k in ('hs', 'cs', 'gates', 'dg'):
            assert torch.equal(full[k][:, b], one[k][:, 0]), (k, b)
        for k in ('hn', 'cn', 'dh0', 'dc0'):
            assert torch.equal(full[k][b], one[k][0]), (k, b)
    assert int(full['err'].item()) == 0


_OUT = ('hs', 'cs', 'gates', 'hn', 'cn', 'dg', 'dh0', 'dc0', 'db')


@pytest.mark.parametrize('shape', [(8, 33, 512), (16, 12, 512)])
def test_wave_gather_repeat_launches(gpu_ops, shape):
    """Three back-to-back forward + backward pairs on one stream, then the same pair captured once and replayed
    three times: every output bitwise equal, error word 0."""
    d = _reference(*shape, False)[0]
    runs = [_launch(gpu_ops, d) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs:
        assert int(r['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(r[k], runs[0][k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # eager run on the capture stream: its control block, allocator
        _launch(gpu_ops, d)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
        cap = _launch(gpu_ops, d)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(cap['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(cap[k], runs[0][k]), k
        for k in _OUT:                          # the next replay has to write them again
            cap[k].zero_()
