"""The forward team recurrence at the start of a chain. The chain-start loads (c0, the bias vector) are landed ahead
of the step loop and the step's prefetch (x·W_ih, the episode-start byte) behind the gather, so that no wait on vector
memory stands between a step's stores and the next step's first poll (ops/csrc/lstm_team_fwd.hip,
profiles/recurrence_fwd_waits.md). A load that was moved wrongly shows where a chain starts: in the first steps, with
non-zero c0 / h0 that differ per row, with an episode start in step 0 or 1, and when a team takes a second chain in
the same launch. Checked against a float64 recurrence with the bounds of tests/test_team_wave_gather.py:

* S = 1, 2, 3, 17 (no, one, two back edges of the step loop, and a longer run) × H = 128, 256, 512 × B = 1, 8 (one
  row per chain), 9 (two), 33 (the eight-row form: seven chains of up to five live rows and an empty eighth) — the
  fp32-exact plan;
* the libm-activation (``precise``) forms of the one-row chains;
* queued launches: more chains than teams, so that a team starts a second chain (its c0 loaded behind a finished one);
* episode starts at t = 0 and t = 1; an all-zero flag tensor bitwise equal to passing none;
* relaunch and hipGraph replay bitwise equal to the first launch; a row bitwise equal to that row launched alone.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SS, HS, BS = (1, 2, 3, 17), (128, 256, 512), (1, 8, 9, 33)
SHAPES = [(B, S, H) for S in SS for H in HS for B in BS]
# (B, S, H, rows per chain): 9 and 17 chains on the 8 teams
QUEUED = [(9, 3, 512, 1), (9, 2, 128, 1), (33, 17, 256, 2), (33, 3, 512, 4)]
FWD_TOL = 2e-5                                  # tests/test_team_wave_gather.py, forward outputs
_OUT = ('hs', 'cs', 'gates', 'hn', 'cn')


def _id(B, S, H, *rest):
    return f'B{B}-S{S}-H{H}' + ''.join(f'-r{r}' for r in rest)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(B, S, H):
    g = torch.Generator(device='cuda').manual_seed(7 + B * 1000 + S * 10 + H)
    return {'xp': torch.randn(S, B, H, 4, device='cuda', generator=g) * 0.5,
            'bias': torch.randn(4 * H, device='cuda', generator=g) * 0.3,
            'whh': torch.randn(4 * H, H, device='cuda', generator=g) * (1.0 / H ** 0.5),
            # non-zero and different in every row: a stale, early or neighbouring c0 / h0 shows in cs[0]
            'h0': torch.randn(B, H, device='cuda', generator=g) * 0.5 + 0.05 * torch.arange(B, device='cuda')[:, None],
            'c0': torch.randn(B, H, device='cuda', generator=g) * 0.7 - 0.03 * torch.arange(B, device='cuda')[:, None]}


def _starts(B, S):
    """(S, B) u8: an episode start at t = 0 in row 0 and at t = 1 in the next row (S = 1: only the first)."""
    r = torch.zeros(S, B, dtype=torch.uint8)
    r[0, 0] = 1
    if S > 1:
        r[1, 1 % B] = 1
    if B > 2 and S > 1:                          # both in one row
        r[0, 2] = 1
        r[1, 2] = 1
    return r.cuda()


def _ref64(d, reset=None):
    """float64 recurrence on unit-major gates (xp (S,B,H,4) time-major, whh (4H,H) gate-major rows)."""
    xp, bias, whh = d['xp'].double(), d['bias'].double(), d['whh'].double()
    S, B, H, _ = xp.shape
    h, c = d['h0'].double(), d['c0'].double()
    hs, cs, gs = [], [], []
    for t in range(S):
        if reset is not None:
            keep = (1.0 - reset[t].double())[:, None]
            h, c = h * keep, c * keep
        pre = xp[t] + bias.view(H, 4) + (h @ whh.t()).view(B, 4, H).transpose(1, 2)
        i, f, gg, o = pre.unbind(-1)
        i, f, o, gg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.stack([i, f, gg, o], -1))
    return {'hs': torch.stack(hs), 'cs': torch.stack(cs), 'gates': torch.stack(gs), 'hn': hs[-1], 'cn': cs[-1]}


_REF = {}


def _reference(B, S, H, with_reset=False):
    """Inputs and float64 outputs of one shape, computed once and shared (read-only)."""
    key = (B, S, H, with_reset)
    if key not in _REF:
        d = _inputs(B, S, H)
        reset = _starts(B, S) if with_reset else None
        _REF[key] = (d, reset, _ref64(d, reset))
    return _REF[key]


def _launch(C, d, reset=None, rows=0, precise=False, row=None):
    from dotaclient_amd.ops.lstm import team_fwd
    sel = (lambda x, dim: x) if row is None else (lambda x, dim: x.narrow(dim, row, 1).contiguous())
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    hs, _, cs, gates, hn, cn = team_fwd(C, sel(d['xp'], 1), d['whh'], sel(d['h0'], 0), sel(d['c0'], 0), err, False,
                                        exact=True, rows=rows, time_major=True, bias4=d['bias'],
                                        reset=None if reset is None else sel(reset, 1), precise=precise)
    return {'hs': hs, 'cs': cs, 'gates': gates, 'hn': hn, 'cn': cn, 'err': err}


def _check(out, ref):
    torch.cuda.synchronize()
    assert int(out['err'].item()) == 0
    # the first step by itself: in a long run its error would drown in the norm of the whole sequence
    assert _rel(out['cs'][0], ref['cs'][0]) < FWD_TOL, ('cs[0]', _rel(out['cs'][0], ref['cs'][0]))
    assert _rel(out['hs'][0], ref['hs'][0]) < FWD_TOL, ('hs[0]', _rel(out['hs'][0], ref['hs'][0]))
    for k in _OUT:
        assert _rel(out[k], ref[k]) < FWD_TOL, (k, _rel(out[k], ref[k]))


@pytest.mark.parametrize('shape', SHAPES, ids=[_id(*s) for s in SHAPES])
def test_chain_start_matches_float64(gpu_ops, shape):
    d, _, ref = _reference(*shape)
    _check(_launch(gpu_ops, d), ref)


PRECISE = [(B, S, H) for S in SS for H in HS for B in (1, 8)]


@pytest.mark.parametrize('shape', PRECISE, ids=[_id(*s) for s in PRECISE])
def test_chain_start_precise_matches_float64(gpu_ops, shape):
    d, _, ref = _reference(*shape)
    _check(_launch(gpu_ops, d, precise=True), ref)


@pytest.mark.parametrize('case', QUEUED, ids=[_id(*c) for c in QUEUED])
def test_chain_start_queued_chains(gpu_ops, case):
    """More chains than teams: a team's second chain loads its c0 and takes its first steps behind a finished chain."""
    from dotaclient_amd.ops.lstm import team_plan
    B, S, H, rows = case
    nch, Bc = team_plan(B, True, True, rows=rows)
    assert nch > 8 and Bc == rows
    d, _, ref = _reference(B, S, H)
    _check(_launch(gpu_ops, d, rows=rows), ref)


STARTS = [(1, 1, 512), (8, 2, 512), (8, 3, 128), (9, 3, 256), (33, 17, 512), (33, 2, 128)]


@pytest.mark.parametrize('shape', STARTS, ids=[_id(*s) for s in STARTS])
def test_chain_start_episode_starts(gpu_ops, shape):
    d, reset, ref = _reference(*shape, True)
    _check(_launch(gpu_ops, d, reset=reset), ref)


@pytest.mark.parametrize('shape', [(8, 2, 512), (9, 3, 128), (33, 17, 256)], ids=lambda s: _id(*s))
def test_chain_start_zero_flags_equal_none(gpu_ops, shape):
    """An all-zero flag tensor and no flag tensor run different paths of the step's prefetch: same bits."""
    d = _reference(*shape)[0]
    a = _launch(gpu_ops, d)
    b = _launch(gpu_ops, d, reset=torch.zeros(shape[1], shape[0], dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    assert int(a['err'].item()) == 0 and int(b['err'].item()) == 0
    for k in _OUT:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('shape', [(8, 3, 512), (3, 2, 128)], ids=lambda s: _id(*s))
def test_chain_start_rows_bitwise_independent(gpu_ops, shape):
    """Both launches run the one-row form: row b among B rows equals row b launched alone, bit for bit."""
    B = shape[0]
    d = _reference(*shape)[0]
    full = _launch(gpu_ops, d)
    for b in range(B):
        one = _launch(gpu_ops, d, row=b)
        torch.cuda.synchronize()
        assert int(one['err'].item()) == 0
        for k in ('hs', 'cs', 'gates'):
            assert torch.equal(full[k][:, b], one[k][:, 0]), (k, b)
        for k in ('hn', 'cn'):
            assert torch.equal(full[k][b], one[k][0]), (k, b)
    assert int(full['err'].item()) == 0


@pytest.mark.parametrize('case', [(8, 17, 512, 0), (33, 3, 256, 0), (9, 3, 512, 1)], ids=lambda c: _id(*c))
def test_chain_start_repeat_launches(gpu_ops, case):
    """Three back-to-back launches, then one captured launch replayed three times: bitwise the first launch."""
    B, S, H, rows = case
    d = _reference(B, S, H)[0]
    runs = [_launch(gpu_ops, d, rows=rows) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs:
        assert int(r['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(r[k], runs[0][k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # eager run on the capture stream: its control block, allocator
        _launch(gpu_ops, d, rows=rows)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
        cap = _launch(gpu_ops, d, rows=rows)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(cap['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(cap[k], runs[0][k]), k
        for k in _OUT:                          # the next replay has to write them again
            cap[k].zero_()
