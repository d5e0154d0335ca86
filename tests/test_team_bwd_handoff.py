"""The exact-fp32 (V1 / V2) team backward with the ∂h hand-off: an owner publishes one {∂h_t, tag} granule per (row,
unit) and every wave of every workgroup turns the granules of its own K part into gate gradients itself, from saved
activations it prefetched, with the cell-gradient carry as per-lane state (ops/csrc/lstm_team_bwd.hip). Checked here,
against the float64 recurrence and with the tolerances of test_team_wave_gather.py: final-state gradients (the
consumer-side carry starts from dcn in every workgroup) at the shapes where the publish-only first iteration, the final
iteration that now also produces ∂gates[0] and ∂c0, lanes without a unit and 2 / 4 rows of per-lane carry can go wrong;
episode starts on consecutive steps (a row's start flags of t and t + 1 set together), at t = 0 and at t = S - 1; row b
of a B-row launch bitwise the row launched alone; relaunches and hipGraph replays bitwise equal with the error word 0."""
import pytest
import torch

from test_team_wave_gather import _g, _inputs, _lstm_ref, _rel

pytestmark = pytest.mark.gpu

# (B, S, H): S = 1 / 2 — publish-only first iteration, final iteration producing ∂gates[0] and ∂c0; H = 128 / 256 —
# lanes without a unit, two K layouts; B = 16 / 32 — two / four rows of per-lane carry
FINAL_SHAPES = [(1, 1, 512), (1, 2, 512), (8, 33, 512), (3, 40, 128), (5, 17, 256), (16, 12, 512), (32, 9, 512)]
START_SHAPES = [(8, 33, 512), (9, 20, 128), (32, 9, 512)]
_GRADS = ('dg', 'dh0', 'dc0', 'db')
_OUT = ('hs', 'cs', 'gates', 'hn', 'cn') + _GRADS


def _finals(B, S, H):
    g = _g(7000 + B * 100 + S)
    return (torch.randn(B, H, device='cuda', generator=g), torch.randn(B, H, device='cuda', generator=g))


def _starts(B, S):
    """(S, B) u8 episode-start flags: t = 0; t = S - 1; two consecutive steps mid-sequence; t = 0, 1 and S - 2, S - 1
    in one row; then a consecutive pair per further row."""
    r = torch.zeros(S, B, dtype=torch.uint8)
    r[0, 0] = 1
    r[S - 1, 1 % B] = 1
    r[S // 2, 2 % B] = r[S // 2 + 1, 2 % B] = 1
    for t in (0, 1, S - 2, S - 1):
        r[t, 3 % B] = 1
    for b in range(4, B):
        t = (5 * b + 3) % S
        r[t, b] = r[min(t + 1, S - 1), b] = 1
    return r.cuda()


def _launch(C, d, dhn=None, dcn=None, reset=None, rows=None):
    """One time-major forward + backward pair; `rows`: that single row launched alone."""
    from dotaclient_amd.ops.lstm import team_bwd, team_fwd
    sel = (lambda x, dim: x) if rows is None else (lambda x, dim: x.narrow(dim, rows, 1).contiguous())
    opt = (lambda x, dim: None if x is None else sel(x, dim))
    h0, c0 = sel(d['h0'], 0), sel(d['c0'], 0)
    rs = opt(reset, 1)
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    hs, _, cs, gates, hn, cn = team_fwd(C, sel(d['xp'], 1), d['whh'], h0, c0, err, False, time_major=True,
                                        bias4=d['bias'], reset=rs)
    dg, dh0, dc0, db = team_bwd(C, sel(d['dh'], 1), gates, cs, c0, opt(dhn, 0), opt(dcn, 0), d['whh'], err,
                                time_major=True, want_dbias=True, reset=rs)
    return {'hs': hs, 'cs': cs, 'gates': gates, 'hn': hn, 'cn': cn, 'dg': dg, 'dh0': dh0, 'dc0': dc0, 'db': db,
            'err': err}


_REF = {}


def _reference(B, S, H, with_finals, with_starts):
    """float64 forward and gradients of one case, computed once and shared (read-only) by the tests that need it."""
    key = (B, S, H, with_finals, with_starts)
    if key not in _REF:
        d = _inputs(B, S, H)
        dhn, dcn = _finals(B, S, H) if with_finals else (None, None)
        reset = _starts(B, S) if with_starts else None
        X = d['xp'].double().requires_grad_(True)
        H0 = d['h0'].double().requires_grad_(True)
        C0 = d['c0'].double().requires_grad_(True)
        hr, cr, gr = _lstm_ref(X, d['bias'].double(), d['whh'].double(), H0, C0,
                               None if reset is None else reset.double())
        loss = (hr * d['dh'].double()).sum()
        if with_finals:
            loss = loss + (hr[-1] * dhn.double()).sum() + (cr[-1] * dcn.double()).sum()
        gx, gh0, gc0 = torch.autograd.grad(loss, [X, H0, C0])
        _REF[key] = (d, dhn, dcn, reset,
                     {'hs': hr.detach(), 'cs': cr.detach(), 'gates': gr.detach(), 'hn': hr[-1].detach(),
                      'cn': cr[-1].detach(), 'dg': gx, 'dh0': gh0, 'dc0': gc0, 'db': gx.sum((0, 1)).t().reshape(-1)})
    return _REF[key]


def _check(out, ref):
    torch.cuda.synchronize()
    assert int(out['err'].item()) == 0
    for k in ('hs', 'cs', 'gates', 'hn', 'cn'):
        assert _rel(out[k], ref[k]) < 2e-5, (k, _rel(out[k], ref[k]))
    for k in _GRADS:
        assert _rel(out[k], ref[k]) < 1e-4, (k, _rel(out[k], ref[k]))


@pytest.mark.parametrize('shape', FINAL_SHAPES)
def test_handoff_final_state_gradients(gpu_ops, shape):
    d, dhn, dcn, _, ref = _reference(*shape, True, False)
    _check(_launch(gpu_ops, d, dhn, dcn), ref)


@pytest.mark.parametrize('shape', START_SHAPES)
def test_handoff_consecutive_episode_starts(gpu_ops, shape):
    d, _, _, reset, ref = _reference(*shape, False, True)
    _check(_launch(gpu_ops, d, reset=reset), ref)


@pytest.mark.parametrize('shape', [(8, 33, 512), (3, 40, 128)])
def test_handoff_rows_bitwise_independent(gpu_ops, shape):
    """Both launches run the one-row instantiation: row b among B rows must equal row b alone, bit for bit."""
    B = shape[0]
    d, dhn, dcn, _, _ = _reference(*shape, True, False)
    full = _launch(gpu_ops, d, dhn, dcn)
    for b in range(B):
        one = _launch(gpu_ops, d, dhn, dcn, rows=b)
        torch.cuda.synchronize()
        assert int(one['err'].item()) == 0
        assert torch.equal(full['dg'][:, b], one['dg'][:, 0]), ('dg', b)
        for k in ('dh0', 'dc0'):
            assert torch.equal(full[k][b], one[k][0]), (k, b)
    assert int(full['err'].item()) == 0


@pytest.mark.parametrize('shape', [(8, 33, 512), (16, 12, 512)])
def test_handoff_repeat_launches(gpu_ops, shape):
    """Three back-to-back forward + backward pairs on one stream, then the same pair captured once and replayed three
    times: every output, ∂b and ∂c0 included, bitwise equal, error word 0."""
    d, dhn, dcn, _, _ = _reference(*shape, True, False)
    runs = [_launch(gpu_ops, d, dhn, dcn) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs:
        assert int(r['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(r[k], runs[0][k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # eager run on the capture stream: its control block, allocator
        _launch(gpu_ops, d, dhn, dcn)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
        cap = _launch(gpu_ops, d, dhn, dcn)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(cap['err'].item()) == 0
        for k in _OUT:
            assert torch.equal(cap[k], runs[0][k]), k
        for k in _OUT:                          # the next replay has to write them again
            cap[k].zero_()
