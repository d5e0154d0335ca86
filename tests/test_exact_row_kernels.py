"""The exact-fp32 row-parallel kernels at the shapes where their tiling can go wrong (not the deploy shape): the
pre-RNN chain kernel in both directions (ops/csrc/dx_chain.hip, EXACT instances: 48-row tiles of three 16-row MFMA
groups, weight slabs staged through three rotating LDS buffers) and the exact encoder backward
(ops/csrc/encoder.hip encoder_bwd_x2_kernel: 16-row items of one unit slot) with the exact encoder forward that
feeds it (encoder_fwd_x_kernel: the same items, taken in pairs). Every case against float64 torch with
the bounds of tests/test_exact_mode.py: 1e-6 relative for activations, max(2e-6, 2 × the torch-fp32 error on the same
inputs) for weight gradients; and every kernel bitwise reproducible (the step's fixed-order sums)."""
import functools

import pytest
import torch

from dotaclient_amd.constants import UnitLayout
from dotaclient_amd.models.policy import TYPE_SUFFIX, Policy, PolicyConfig

# a partial 16-row group, exactly one group, one row into the next; one row short of a tile, exactly one tile, one
# row into the next tile; three tiles (fewer than CUs); 15 tiles with a partial last one
CHAIN_N = [1, 15, 16, 17, 47, 48, 49, 97, 700]
P, X896, G4 = 256, 896, 2048


def _rel(a, b):
    return ((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _chain_weights():
    g = torch.Generator().manual_seed(1)
    wpre = torch.randn(P, X896, generator=g, dtype=torch.float64) * 0.03
    wih = torch.randn(G4, P, generator=g, dtype=torch.float64) * 0.06
    bpre = torch.randn(P, generator=g, dtype=torch.float64) * 0.1
    return wpre, wih, bpre


@functools.lru_cache(maxsize=None)
def _chain_case(N):
    """Inputs (float64, exactly representable in fp32) and the float64 results of both chain directions."""
    wpre, wih, bpre = (t.float().double() for t in _chain_weights())
    g = torch.Generator().manual_seed(100 + N)
    x896 = torch.randn(N, X896, generator=g).double()
    x = torch.relu(x896 @ wpre.t() + bpre)
    xp = x @ wih.t()
    dG = torch.randn(N, G4, generator=g).double()
    xm = torch.relu(torch.randn(N, P, generator=g)).double()      # the layer's output as saved by the forward: ≥ 0
    dpre = (dG @ wih) * (xm > 0)
    dx = dpre @ wpre
    return dict(x896=x896, x=x, xp=xp, dG=dG, xm=xm, dpre=dpre, dx=dx)


def _dev(t):
    return t.float().cuda().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('N', CHAIN_N)
def test_exact_forward_chain_matches_fp64(gpu_ops, N):
    """x = relu(x896·W_preᵀ + b), xp = x·W_ihᵀ (pre_rnn_chain, exact) against float64; bitwise reproducible."""
    C = gpu_ops
    wpre, wih, bpre = _chain_weights()
    c = _chain_case(N)
    nil = torch.empty(0, device='cuda')
    args = (_dev(c['x896']), _dev(wpre), nil, _dev(bpre), _dev(wih), nil)
    x, xp = C.pre_rnn_chain(*args)
    x2, xp2 = C.pre_rnn_chain(*args)
    torch.cuda.synchronize()
    ex, exp = _rel(x, c['x']), _rel(xp, c['xp'])
    print(f'forward chain N={N}: x {ex:.3e} xp {exp:.3e}')
    assert x.shape == (N, P) and xp.shape == (N, G4)
    assert ex < 1e-6 and exp < 1e-6
    assert torch.equal(x, x2) and torch.equal(xp, xp2)


@pytest.mark.gpu
@pytest.mark.parametrize('N', CHAIN_N)
def test_exact_dx_chain_matches_fp64(gpu_ops, N):
    """dpre = (dG·W_ih) ⊙ [x > 0], dx = dpre·W_pre (dpre_dx, exact) against float64; dpre exactly zero where the
    layer's output is zero; bitwise reproducible."""
    C = gpu_ops
    wpre, wih, _ = _chain_weights()
    c = _chain_case(N)
    nil = torch.empty(0, device='cuda')
    xm = _dev(c['xm'])
    args = (_dev(c['dG']), _dev(wih.t()), nil, xm, _dev(wpre.t()), nil)
    dpre, dx = C.dpre_dx(*args)
    dpre2, dx2 = C.dpre_dx(*args)
    torch.cuda.synchronize()
    ep, ed = _rel(dpre, c['dpre']), _rel(dx, c['dx'])
    print(f'dX chain N={N}: dpre {ep:.3e} dx {ed:.3e}')
    assert dpre.shape == (N, P) and dx.shape == (N, X896)
    assert ep < 1e-6 and ed < 1e-6
    assert (dpre[xm == 0] == 0).all()
    assert torch.equal(dpre, dpre2) and torch.equal(dx, dx2)


# lstm512's unit counts, and a layout of odd counts (item runs of a type end on odd item numbers, so a pair of
# consecutive items straddles a type boundary and a job can end on a single item)
ENC_LAYOUTS = {'lstm512': UnitLayout(), 'odd': UnitLayout(3, 5, 7, 9, 1, 3)}
ZERO_TYPE = 4          # 'odd': this type's incoming gradient is exactly zero


def _ref_encoder(pol, units, env):
    """Policy.encode up to x896 with max pooling (the construction of tests/test_exact_mode.py)."""
    import torch.nn.functional as F
    from dotaclient_amd.constants import UNIT_KEYS
    env_e = F.relu(pol.affine_env(env))
    basic = F.relu(pol.affine_unit_basic_stats(units))
    sl = pol.layout.slices()
    emb = torch.cat([getattr(pol, f'affine_unit_{s}')(basic[:, sl[k]]) for k, s in zip(UNIT_KEYS, TYPE_SUFFIX)], 1)
    pools = [emb[:, sl[k]].max(dim=1).values for k in UNIT_KEYS]
    return torch.cat([env_e] + pools, 1), emb


@functools.lru_cache(maxsize=None)
def _enc_case(name, N):
    """Inputs, float64 gradients and the torch-fp32 gradients (the round-off yardstick) of one encoder case."""
    from dotaclient_amd.constants import UNIT_KEYS
    torch.manual_seed(0)
    cfg = PolicyConfig(rnn='lstm', hidden=512, layout=ENC_LAYOUTS[name])
    pol = Policy(cfg).double()
    U = pol.layout.max_units
    g = torch.Generator().manual_seed(7 * N + len(name))
    units = torch.randn(N, U, 10, generator=g).double()
    env = torch.randn(N, 3, generator=g).double()
    dx = torch.randn(N, 896, generator=g).double()
    dtl = torch.randn(N, U, generator=g).double()
    z = torch.randn(N, 160, generator=g).double()
    if name == 'odd':
        dtl[:, pol.layout.slices()[UNIT_KEYS[ZERO_TYPE]]] = 0
        dx[:, 128 * (1 + ZERO_TYPE):128 * (2 + ZERO_TYPE)] = 0
    names = ['affine_unit_basic_stats.weight', 'affine_unit_basic_stats.bias'] + \
        [f'affine_unit_{s}.weight' for s in TYPE_SUFFIX]

    def grads(p, cast):
        Pm = dict(p.named_parameters())
        xr, er = _ref_encoder(p, cast(units), cast(env))
        demb = cast(dtl).unsqueeze(2) * cast(z)[:, None, :128]
        return dict(zip(names, torch.autograd.grad([xr, er], [Pm[n] for n in names], grad_outputs=[cast(dx), demb])))
    g64 = grads(pol, lambda t: t)
    with torch.no_grad():
        x64, e64 = _ref_encoder(pol, units, env)
    pol32 = Policy(cfg).float()
    pol32.load_state_dict({k: v.float() for k, v in pol.state_dict().items()})
    g32 = grads(pol32, lambda t: t.float())
    return dict(pol=pol, units=units, env=env, dx=dx, dtl=dtl, z=z, g64=g64, g32=g32, x64=x64, e64=e64)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [1, 16, 17, 33, 500])
@pytest.mark.parametrize('name', list(ENC_LAYOUTS))
def test_exact_encoder_fwd_matches_fp64(gpu_ops, name, N):
    """x896 and the unit embeddings of the exact encoder forward (items taken in pairs, an odd last item apart)
    against float64; bitwise reproducible, argmax included."""
    C = gpu_ops
    c = _enc_case(name, N)
    pol = c['pol']
    Pm = dict(pol.named_parameters())
    f = lambda t: t.detach().float().cuda().contiguous()       # noqa: E731
    wt = torch.stack([f(Pm[f'affine_unit_{s}.weight']) for s in TYPE_SUFFIX])
    bt = torch.stack([f(Pm[f'affine_unit_{s}.bias']) for s in TYPE_SUFFIX])
    args = (f(c['units']), f(c['env']), f(Pm['affine_unit_basic_stats.weight']), f(Pm['affine_unit_basic_stats.bias']),
            wt, bt, f(Pm['affine_env.weight']), f(Pm['affine_env.bias']), list(pol.layout.counts), False)
    x896, emb, arg = C.encoder_fwd(*args, exact=True)
    x2, emb2, arg2 = C.encoder_fwd(*args, exact=True)
    torch.cuda.synchronize()
    ex, ee = _rel(x896, c['x64']), _rel(emb, c['e64'])
    print(f'encoder fwd {name} N={N}: x896 {ex:.3e} emb {ee:.3e}')
    assert ex < 1e-6 and ee < 1e-6
    assert torch.equal(x896, x2) and torch.equal(emb, emb2) and torch.equal(arg, arg2)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [1, 16, 17, 33, 500])
@pytest.mark.parametrize('name', list(ENC_LAYOUTS))
def test_exact_encoder_bwd_matches_fp64(gpu_ops, name, N):
    """∂W_τ, ∂W1, ∂b1 of the exact encoder backward against float64 autograd; a type whose incoming gradient is zero
    gets an exactly zero ∂W_τ; bitwise reproducible."""
    C = gpu_ops
    c = _enc_case(name, N)
    pol = c['pol']
    Pm = dict(pol.named_parameters())
    counts = list(pol.layout.counts)
    f = lambda t: t.detach().float().cuda().contiguous()       # noqa: E731
    wt = torch.stack([f(Pm[f'affine_unit_{s}.weight']) for s in TYPE_SUFFIX])
    bt = torch.stack([f(Pm[f'affine_unit_{s}.bias']) for s in TYPE_SUFFIX])
    w1, b1 = f(Pm['affine_unit_basic_stats.weight']), f(Pm['affine_unit_basic_stats.bias'])
    units = f(c['units'])
    _, _, arg = C.encoder_fwd(units, f(c['env']), w1, b1, wt, bt, f(Pm['affine_env.weight']), f(Pm['affine_env.bias']),
                              counts, False, exact=True)
    args = (units, w1, b1, wt.transpose(1, 2).contiguous(), f(c['dtl']), f(c['z']), f(c['dx']), arg, counts, False)
    dwt, dw1, db1 = C.encoder_bwd(*args, exact=True)
    dwt2, dw1b, db1b = C.encoder_bwd(*args, exact=True)
    torch.cuda.synchronize()
    g64, g32 = c['g64'], c['g32']
    rows = [('dW1', dw1, 'affine_unit_basic_stats.weight'), ('db1', db1, 'affine_unit_basic_stats.bias')] + \
        [(f'dW_{s}', dwt[t], f'affine_unit_{s}.weight') for t, s in enumerate(TYPE_SUFFIX)]
    for label, got, n in rows:
        if name == 'odd' and label == f'dW_{TYPE_SUFFIX[ZERO_TYPE]}':
            assert g64[n].abs().max().item() == 0.0
            assert got.abs().max().item() == 0.0, label
            continue
        e, e32 = _rel(got, g64[n]), _rel(g32[n], g64[n])
        print(f'encoder bwd {name} N={N} {label}: {e:.3e} (torch fp32 {e32:.3e})')
        assert e <= max(2e-6, 2 * e32), label
    assert torch.equal(dwt, dwt2) and torch.equal(dw1, dw1b) and torch.equal(db1, db1b)
