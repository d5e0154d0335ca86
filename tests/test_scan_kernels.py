"""The learner's scan kernels (ops/csrc/scan.hip) directly against float64.

``vtrace_step_kernel`` (V-trace inside the learner step) and ``returns_scan_kernel`` + ``ema_normalize_kernel`` (the
per-iteration return / GAE / V-trace scan) are chunked linear recurrences: every thread reduces its rows to an affine
map, the maps are composed by a wave suffix scan and an LDS pass over the four waves, and every thread replays its rows
from its carry. The tests run them at every sequence length where that structure changes (one row per thread, the
256-thread boundary, several rows per thread, ragged last chunks, empty segments) in two ways:

* exact cases: dyadic inputs (multiples of 1/8), unit discount and importance weights clipped to exactly 1, so every
  partial result is representable in fp32 in any association order and the kernel must reproduce the float64 result
  bit for bit; a wrong chunk boundary, carry or dropped partial shows as an inequality, with no tolerance to hide in;
* tolerance cases: random inputs, default discounts, (ρ̄, c̄) = (1, 1) and (2, 0.5), per element
  |got − ref| ≤ 1e-5 · max(1, max|ref|) (the fp32 recurrence itself measures ≈ 2e-7 of max|A|; the rest is the
  hardware exponential of the importance weights).

The CPU tests pin the two torch oracles themselves to closed forms (telescoping sums) written without the recursion.
"""
import functools

import numpy as np
import pytest
import torch

from dotaclient_amd.ops.scan import compute_returns, vtrace_step

VT_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 350, 511, 512, 513, 1000]
VCOL = 149
TOL = 1e-5


def _dyadic(gen, shape, lo, hi, den=8):
    """Multiples of 1/den in [lo, hi] (float32, exactly representable)."""
    return torch.randint(int(lo * den), int(hi * den) + 1, shape, generator=gen).float() / den


# ---- vtrace_step: inputs ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vt_exact_inputs(S, B):
    """Dyadic time-major rows with γ = λ = 1 and mu = lp − 1 (w = e > 1 = ρ̄ = c̄: ρ = c = 1 whatever the exponential's
    accuracy). Sequence b % 3 == 0: no inner `last`, no invalid row (the carry crosses every thread and wave boundary);
    1: a `last` in the middle; 2: an invalid tail (not closed by a `last`). The bootstrap column is nonzero on EVERY row,
    so using it anywhere but at a `last` row shows."""
    g = torch.Generator().manual_seed(1000 * S + B)
    r, boot, V = _dyadic(g, (S, B), -2, 2), _dyadic(g, (S, B), -2, 2), _dyadic(g, (S, B), -2, 2)
    lp = _dyadic(g, (S, B), -4, 0)
    valid, last = torch.ones(S, B), torch.zeros(S, B)
    for b in range(B):
        if b % 3 == 1 and S >= 2:
            last[S // 2 - 1, b] = 1.0
        if b % 3 == 2 and S >= 2:
            valid[S - max(1, S // 5):, b] = 0.0
    vt = torch.stack([r, boot, valid, last], -1)
    return {'V': V.reshape(-1), 'lp': lp.reshape(-1), 'mu': (lp - 1.0).reshape(-1), 'vt': vt.reshape(-1, 4).contiguous()}


@functools.lru_cache(maxsize=None)
def _vt_random_inputs(S, B):
    """The pattern of tests/test_offpolicy.py::_vt_batch: `last` with probability 0.04 plus the final row, bootstrap
    values at the `last` rows, an invalid tail of up to S/5 rows in odd sequences, mu = lp + 0.5·randn."""
    g = torch.Generator().manual_seed(7000 * S + B)
    last = (torch.rand(S, B, generator=g) < 0.04).float()
    last[-1] = 1.0
    r = torch.randn(S, B, generator=g) * 0.3
    boot = torch.randn(S, B, generator=g) * last
    valid = torch.ones(S, B)
    for b in range(1, B, 2):
        if S // 5 >= 1:
            valid[S - int(torch.randint(1, S // 5 + 1, (1,), generator=g)):, b] = 0.0
    V = torch.randn(S, B, generator=g)
    lp = -(torch.rand(S, B, generator=g) * 2.0 + 0.5)
    mu = lp + 0.5 * torch.randn(S, B, generator=g)
    vt = torch.stack([r, boot, valid, last], -1)
    return {'V': V.reshape(-1), 'lp': lp.reshape(-1), 'mu': mu.reshape(-1), 'vt': vt.reshape(-1, 4).contiguous()}


def _vt_ref(c, B, S, gamma, lam, rho_bar, c_bar):
    """The torch path evaluated in float64 (its inputs are cast up before the first operation)."""
    return vtrace_step(c['V'].double(), c['lp'].double(), c['mu'].double(), c['vt'].double(), B, S, gamma, lam,
                       rho_bar, c_bar)


def _vt_closed_form(c, B, S):
    """γ = λ = ρ = c = 1: A_t = Σ_{s=t..e} r_s + bootstrap_e − V_t over the valid rows, where the episode segment of t
    ends at e = the first row ≥ t that is a `last` row, the sequence's final row, or the row before an invalid one; its
    bootstrap is vt[e].bootstrap at a `last` / final row and the next row's value otherwise. Written as explicit sums."""
    V = c['V'].double().reshape(S, B)
    v4 = c['vt'].double().reshape(S, B, 4)
    A = torch.zeros(S, B, dtype=torch.float64)
    for b in range(B):
        for t in range(S):
            if v4[t, b, 2] <= 0:
                continue
            e = t
            while not (v4[e, b, 3] > 0 or e == S - 1 or v4[e + 1, b, 2] <= 0):
                e += 1
            boot = v4[e, b, 1] if (v4[e, b, 3] > 0 or e == S - 1) else V[e + 1, b]
            A[t, b] = v4[t:e + 1, b, 0].sum() + boot - V[t, b]
    valid = v4[..., 2] > 0
    ret = torch.where(valid, A + V, torch.zeros_like(V))
    return A.reshape(-1), ret.reshape(-1), valid.double().sum(0)


# ---- CPU: the oracles against closed forms ---------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 2, 65, 257, 350])
def test_vtrace_step_oracle_telescopes(S):
    """ops.scan.vtrace_step (torch path) at γ = λ = 1, ρ̄ = c̄ = 1, mu = lp − 1 equals the telescoped sum exactly (dyadic
    inputs: every float64 operation is exact), the sum is cut at `last` rows and A is 0 on invalid rows."""
    B = 3
    c = _vt_exact_inputs(S, B)
    adv, ret, stats = _vt_ref(c, B, S, 1.0, 1.0, 1.0, 1.0)
    A, R, nv = _vt_closed_form(c, B, S)
    assert torch.equal(adv.double(), A) and torch.equal(ret.double(), R)
    invalid = c['vt'][:, 2] <= 0
    assert (adv[invalid] == 0).all() and (ret[invalid] == 0).all()
    assert torch.equal(stats.double(), torch.stack([nv, nv, -nv, nv], 1))
    if S >= 2:      # the three kinds of sequence really differ: a cut changes the rows before it
        assert bool(invalid.any()) and float(c['vt'][:, 3].sum()) >= 1


SEG_LENGTHS = [0, 1, 255, 256, 257, 511, 512, 513, 1000]
SEQ = 16


def _seg_case(lens, K, seed, dyadic, keys=None, n_keys=3):
    """Concatenated rollouts, each padded to a multiple of 16 rows and to at least one sequence. Rewards are nonzero in
    the padding too (the `discount` mode scans it). Dyadic: rewards ≥ 0 and sparse enough that every sum of returns
    stays below 2^24 / 8, so the kernel's fp32 sums are exact and the segment means are > 0 (no cancellation in the
    statistics); the resumed EMA row is dyadic and positive."""
    g = torch.Generator().manual_seed(seed)
    padded = [max(SEQ, -(-T // SEQ) * SEQ) for T in lens]
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int32)
    L, n = int(off[-1]), len(lens)
    if dyadic:
        rew = _dyadic(g, (L, K), 0, 0.125) * (torch.rand(L, K, generator=g) < min(1.0, 6.0 / K)).float()
        val, boot = _dyadic(g, (L,), -2, 2), _dyadic(g, (n,), -2, 2)
    else:
        rew, val, boot = torch.randn(L, K, generator=g) * 0.1, torch.randn(L, generator=g), torch.randn(n, generator=g)
    done = [bool(i % 3 == 0) for i in range(n)]
    if keys is None:
        keys = [(i * 5 // 3) % 2 for i in range(n)]             # two keys, interleaved irregularly
    ema = torch.zeros(n_keys, 3)
    ema[1] = torch.tensor([0.375, 1.5, 1.0])                    # key 1 resumes a nonzero state, key 0 starts fresh
    lr_rand = torch.randn(L, generator=g) * 0.5
    return {'rew': rew, 'val': val, 'off': off, 'lens': list(lens), 'boot': boot, 'done': done, 'keys': keys,
            'ema': ema, 'lr': torch.ones(L) if dyadic else lr_rand}


def _returns(c, mode, device, double=False, **kw):
    """compute_returns on `device`; double=True feeds the CPU reference float64 inputs."""
    cast = (lambda t: t.double()) if double else (lambda t: t.to(device))
    ema = cast(c['ema'].clone())
    out = compute_returns(cast(c['rew']), cast(c['val']), c['off'], c['lens'], c['boot'], c['done'], c['keys'], ema,
                          mode, lr=cast(c['lr']), **kw)
    return out, ema


@pytest.mark.parametrize('mode', ['discount', 'gae', 'vtrace'])
def test_compute_returns_oracle_telescopes(mode):
    """ops.scan._reference at γ = λ = 1 (vtrace: lr = +1, ρ̄ = c̄ = 1): A_t = Σ_{s=t..T−1} r_s + bootstrap − V_t with
    ret = A + V and zeros in the padding; `discount`: G_t is the plain suffix sum over the padded segment. Exact."""
    c = _seg_case([0, 1, 15, 16, 17, 40], 9, 5, dyadic=True)
    out, _ = _returns(c, mode, 'cpu', double=True, gamma=1.0, lam=1.0, normalize=False)
    r = c['rew'].double().sum(1)
    v = c['val'].double()
    for s, T in enumerate(c['lens']):
        a, b = int(c['off'][s]), int(c['off'][s + 1])
        if mode == 'discount':
            G = torch.flip(torch.cumsum(torch.flip(r[a:b], [0]), 0), [0])
            assert torch.equal(out['ret'][a:b].double(), G) and torch.equal(out['adv'][a:b].double(), G)
            continue
        boot = 0.0 if c['done'][s] else float(c['boot'][s])
        A = torch.stack([r[a + t:a + T].sum() + boot - v[a + t] for t in range(T)]) if T else r[:0]
        assert torch.equal(out['adv'][a:a + T].double(), A)
        assert torch.equal(out['ret'][a:a + T].double(), A + v[a:a + T])
        assert (out['ret'][a + T:b] == 0).all() and (out['adv'][a + T:b] == 0).all()


# ---- GPU: vtrace_step_kernel -----------------------------------------------------------------------------------------
def _vt_kernel(c, B, S, ldz, gamma, lam, rho_bar, c_bar):
    g = torch.Generator().manual_seed(S * 31 + ldz)
    z = torch.randn(B * S, ldz, generator=g)
    z[:, VCOL] = c['V']
    z = z.cuda()
    out = vtrace_step(None, c['lp'].cuda(), c['mu'].cuda(), c['vt'].cuda(), B, S, gamma, lam, rho_bar, c_bar, z=z,
                      vcol=VCOL)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize('S', VT_LENGTHS)
def test_vtrace_step_kernel_exact(gpu_ops, S):
    """Dyadic inputs, γ = λ = 1, mu = lp − 1: adv and ret bitwise equal to float64 and stats exactly
    {n_valid, n_valid, −n_valid, n_valid}, at every chunking of the sequence (one row per thread up to S = 256, then
    2-4 rows per thread with a ragged last chunk), B ∈ {1, 3}, row strides 160 and 256."""
    for B in (1, 3):
        c = _vt_exact_inputs(S, B)
        adv_ref, ret_ref, st_ref = _vt_ref(c, B, S, 1.0, 1.0, 1.0, 1.0)
        nv = (c['vt'][:, 2] > 0).float().reshape(S, B).sum(0)
        assert torch.equal(st_ref, torch.stack([nv, nv, -nv, nv], 1))
        for ldz in (160, 256):
            adv, ret, stats = _vt_kernel(c, B, S, ldz, 1.0, 1.0, 1.0, 1.0)
            bad = (adv != adv_ref).nonzero().flatten().tolist()
            assert not bad, f'adv differs at rows {bad[:8]} (S={S} B={B} ldz={ldz})'
            assert torch.equal(ret, ret_ref), f'ret S={S} B={B} ldz={ldz}'
            assert torch.equal(stats, st_ref), f'stats S={S} B={B} ldz={ldz}: {stats.tolist()}'
            assert (ret[c['vt'][:, 2] <= 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('bars', [(1.0, 1.0), (2.0, 0.5)], ids=['rho1_c1', 'rho2_c0.5'])
@pytest.mark.parametrize('S', VT_LENGTHS)
def test_vtrace_step_kernel_matches_float64(gpu_ops, S, bars):
    """Random rows, γ = 0.98, λ = 0.95: per element |got − ref| ≤ 1e-5 · max(1, max|ref|) for adv and ret, every stats
    sum within 1e-5 × the float64 sum of the absolute values of its terms, ret exactly 0 on invalid rows."""
    rho_bar, c_bar = bars
    worst = 0.0
    for B in (1, 3):
        c = _vt_random_inputs(S, B)
        adv_ref, ret_ref, _ = _vt_ref(c, B, S, 0.98, 0.95, rho_bar, c_bar)
        v4 = c['vt'].double().reshape(S, B, 4)
        valid = (v4[..., 2] > 0).double()
        dl = (c['lp'].double() - c['mu'].double()).reshape(S, B)
        w = torch.exp(dl)
        trunc = (w > rho_bar * (1 + 1e-6)).double()
        if S >= 64 and B == 3:              # the case really has what it is meant to exercise
            assert 0 < float((trunc * valid).sum()) < float(valid.sum())
            assert float(v4[:-1, :, 3].sum()) >= 1 and float((1 - valid).sum()) >= 1
        # no weight so close to the threshold that the hardware exponential could flip the truncation count
        assert float((w / (rho_bar * (1 + 1e-6)) - 1).abs().min()) > 3e-6
        terms = [w.clamp(max=rho_bar) * valid, trunc * valid, -dl * valid, valid]
        st_ref = torch.stack([t.sum(0) for t in terms], 1)
        st_mag = torch.stack([t.abs().sum(0) for t in terms], 1)
        for ldz in (160, 256):
            adv, ret, stats = _vt_kernel(c, B, S, ldz, 0.98, 0.95, rho_bar, c_bar)
            for name, got, ref in (('adv', adv, adv_ref), ('ret', ret, ret_ref)):
                scale = max(1.0, float(ref.abs().max()))
                err = float((got.double() - ref.double()).abs().max()) / scale
                worst = max(worst, err)
                assert err <= TOL, f'{name} S={S} B={B} ldz={ldz}: {err:.3e}'
            serr = float(((stats.double() - st_ref).abs() / st_mag.clamp_min(1e-30)).max())
            assert serr <= TOL, f'stats S={S} B={B} ldz={ldz}: {serr:.3e}'
            assert (ret[c['vt'][:, 2] <= 0] == 0).all()
    print(f'vtrace_step S={S} rho_bar={rho_bar} c_bar={c_bar}: worst |err|/max(1,max|ref|) = {worst:.3e} '
          f'(bound {TOL:.0e})')


# ---- GPU: returns_scan_kernel + ema_normalize_kernel through compute_returns ----------------------------------------------
def _check_exact(c, mode, **kw):
    """ret / adv bitwise the float64 reference; the statistics and the EMA state (one fp32 division and a square root,
    a convex fold with the dyadic factor 0.5) to 1e-6 relative. In `discount` mode with normalisation `adv` is the
    normalised return (G − μ)/(σ + eps), which no input makes exact: it is held to 1e-5 there and `ret` stays bitwise;
    with normalize=False `adv` is `ret` and both are bitwise."""
    ref, ema_ref = _returns(c, mode, 'cpu', double=True, gamma=1.0, lam=1.0, factor=0.5, **kw)
    got, ema = _returns(c, mode, 'cuda', gamma=1.0, lam=1.0, factor=0.5, **kw)
    torch.cuda.synchronize()
    normalised = mode == 'discount' and kw.get('normalize', True)
    if normalised:
        torch.testing.assert_close(got['adv'].cpu(), ref['adv'], rtol=TOL, atol=TOL)
    for k in ('ret',) if normalised else ('ret', 'adv'):
        bad = (got[k].cpu() != ref[k]).nonzero().flatten().tolist()
        assert not bad, f'{k} differs at rows {bad[:8]}'
    torch.testing.assert_close(got['stats'].cpu(), ref['stats'], rtol=1e-6, atol=0)
    torch.testing.assert_close(ema.cpu().double(), ema_ref, rtol=1e-6, atol=0)


def _check_close(c, mode, label, keys=('ret', 'adv', 'norm', 'stats'), **kw):
    ref, ema_ref = _returns(c, mode, 'cpu', double=True, **kw)
    got, ema = _returns(c, mode, 'cuda', **kw)
    torch.cuda.synchronize()
    errs = {}
    for k in ('ret', 'adv'):
        scale = max(1.0, float(ref[k].abs().max()))
        errs[k] = float((got[k].cpu().double() - ref[k].double()).abs().max()) / scale
    for k in ('norm', 'stats'):
        if k in keys:
            errs[k] = float((got[k].cpu().double() - ref[k].double()).abs().max())
    errs['ema'] = float((ema.cpu().double() - ema_ref).abs().max())
    print(f'returns_scan {label}: ' + ' '.join(f'{k} {v:.3e}' for k, v in errs.items()) + f' (bound {TOL:.0e})')
    assert errs['ret'] <= TOL and errs['adv'] <= TOL, errs
    for k in ('norm', 'stats'):
        if k in keys:
            torch.testing.assert_close(got[k].cpu(), ref[k], rtol=TOL, atol=TOL, msg=f'{label} {k}')
    torch.testing.assert_close(ema.cpu().double(), ema_ref, rtol=TOL, atol=TOL, msg=f'{label} ema')
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 9, 64])
@pytest.mark.parametrize('mode', ['discount', 'gae', 'vtrace'])
def test_returns_scan_kernel_exact(gpu_ops, mode, K):
    """Segments of 0, 1 and every length around the 256-thread chunk boundaries, dyadic rewards / values, γ = λ = 1
    (vtrace: lr = +1, so ρ = c = 1): ret and adv bitwise equal to float64."""
    _check_exact(_seg_case(SEG_LENGTHS, K, 11 + K, dyadic=True), mode)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 9, 64])
@pytest.mark.parametrize('mode', ['discount', 'gae', 'vtrace'])
def test_returns_scan_kernel_matches_float64(gpu_ops, mode, K):
    _check_close(_seg_case(SEG_LENGTHS, K, 23 + K, dyadic=False), mode, f'{mode} K={K}')


@pytest.mark.gpu
def test_returns_scan_kernel_other_cases(gpu_ops):
    """normalize=False (discount), clipped weights (ρ̄, c̄) = (2, 0.5) (vtrace), a single-segment call, and 200
    segments of one key (the serial EMA fold in rollout order)."""
    c = _seg_case(SEG_LENGTHS, 9, 31, dyadic=False)
    got = _check_close(c, 'discount', 'discount normalize=False', keys=('ret', 'adv', 'stats'), normalize=False)
    assert torch.equal(got['adv'], got['ret'])
    _check_exact(_seg_case(SEG_LENGTHS, 9, 32, dyadic=True), 'discount', normalize=False)
    _check_close(c, 'vtrace', 'vtrace rho_bar=2 c_bar=0.5', rho_bar=2.0, c_bar=0.5)
    for mode in ('discount', 'gae', 'vtrace'):
        _check_close(_seg_case([300], 9, 33, dyadic=False, keys=[1]), mode, f'{mode} single segment')
        _check_exact(_seg_case([513], 9, 34, dyadic=True, keys=[0]), mode)
        lens = [1 + (7 * i) % 16 for i in range(200)]
        _check_close(_seg_case(lens, 9, 35, dyadic=False, keys=[1] * 200), mode, f'{mode} 200 segments of one key')
