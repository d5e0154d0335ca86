"""The fp32-exact learner mode (FusedPolicy(precision='fp32-exact')): IEEE-fp32 products end to end, every product
on a hand-written kernel (v_mfma_f32_16x16x4_f32 / fp32 VALU), no vendor GEMM.

GPU: the exact entity-encoder kernels (ops/csrc/encoder.hip encoder_fwd_x_kernel / encoder_bwd_x_kernel) against
float64 autograd through the reference encoder (Policy.encode with the reference's ``max`` pooling,
/root/reference/policy.py:97-132); the whole fused step at the deploy shape (lstm512, B=8, S=1400) against a float64
evaluation, per tensor."""
import pytest
import torch

from dotaclient_amd.models.policy import TYPE_SUFFIX, Policy, get_config


class _FP:
    def __init__(self, cfg):
        self.cfg = cfg


def _ref_encoder(pol, units, env):
    """Policy.encode up to x896, with max (argmax-routed gradient) pooling like the reference (policy.py:102-127)."""
    import torch.nn.functional as F
    from dotaclient_amd.constants import UNIT_KEYS
    cfg = pol.config
    env_e = F.relu(pol.affine_env(env))
    basic = F.relu(pol.affine_unit_basic_stats(units))
    sl = pol.layout.slices()
    emb = torch.cat([getattr(pol, f'affine_unit_{s}')(basic[:, sl[k]]) for k, s in zip(UNIT_KEYS, TYPE_SUFFIX)], 1)
    pools = []
    for k in UNIT_KEYS:
        kk = 'enemy_nonheroes' if (cfg.compat_bugs and k == 'enemy_towers') else k
        pools.append(emb[:, sl[kk]].max(dim=1).values)
    return torch.cat([env_e] + pools, 1), emb


@pytest.mark.gpu
@pytest.mark.parametrize('preset,N', [('lstm512', 1000), ('compat', 333)])
def test_exact_encoder_kernels_match_autograd_fp64(gpu_ops, preset, N):
    """x896 / emb / argmax forward and ∂W_τ, ∂W1, ∂b1 backward of the exact encoder kernels: within fp32 round-off of
    float64 (and at least as close as the same encoder evaluated by torch in fp32)."""
    C = gpu_ops
    torch.manual_seed(0)
    pol = Policy(get_config(preset)).double()
    cfg = pol.config
    U = pol.layout.max_units
    dev = torch.device('cuda')
    units = torch.randn(N, U, 10, dtype=torch.float64)
    env = torch.randn(N, 3, dtype=torch.float64)
    dx = torch.randn(N, 896, dtype=torch.float64)
    dtl = torch.randn(N, U, dtype=torch.float64)
    z = torch.randn(N, 160, dtype=torch.float64)
    P = dict(pol.named_parameters())
    xr, er = _ref_encoder(pol, units, env)
    demb = dtl.unsqueeze(2) * z[:, None, :128]
    names = ['affine_unit_basic_stats.weight', 'affine_unit_basic_stats.bias'] + \
        [f'affine_unit_{s}.weight' for s in TYPE_SUFFIX]
    g = dict(zip(names, torch.autograd.grad([xr, er], [P[n] for n in names], grad_outputs=[dx, demb],
                                            allow_unused=True)))
    f = lambda t: t.detach().float().to(dev).contiguous()       # noqa: E731
    wt = torch.stack([f(P[f'affine_unit_{s}.weight']) for s in TYPE_SUFFIX])
    bt = torch.stack([f(P[f'affine_unit_{s}.bias']) for s in TYPE_SUFFIX])
    counts = list(cfg.layout.counts)
    x896, emb, arg = C.encoder_fwd(f(units), f(env), f(P['affine_unit_basic_stats.weight']),
                                   f(P['affine_unit_basic_stats.bias']), wt, bt, f(P['affine_env.weight']),
                                   f(P['affine_env.bias']), counts, bool(cfg.compat_bugs), exact=True)
    if cfg.compat_bugs:                       # the learner applies the reference's eth = enh pool fix-up itself
        x896[:, 768:896] = x896[:, 512:640]
        arg[:, 5] = arg[:, 3]
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()
    assert rel(x896, xr.detach()) < 1e-6
    assert rel(emb, er.detach()) < 1e-6
    dwt, dw1, db1 = C.encoder_bwd(f(units), f(P['affine_unit_basic_stats.weight']),
                                  f(P['affine_unit_basic_stats.bias']), wt.transpose(1, 2).contiguous(), f(dtl), f(z),
                                  f(dx), arg, counts, bool(cfg.compat_bugs), exact=True)
    torch.cuda.synchronize()
    # torch fp32 evaluation of the same gradients: the round-off yardstick
    pol32 = Policy(cfg).float()
    pol32.load_state_dict({k: v.float() for k, v in pol.state_dict().items()})
    P32 = dict(pol32.named_parameters())
    xr32, er32 = _ref_encoder(pol32, units.float(), env.float())
    g32 = dict(zip(names, torch.autograd.grad([xr32, er32], [P32[n] for n in names],
                                              grad_outputs=[dx.float(), demb.float()], allow_unused=True)))
    assert rel(dw1, g['affine_unit_basic_stats.weight']) <= max(2e-6, 2 * rel(g32['affine_unit_basic_stats.weight'],
                                                                               g['affine_unit_basic_stats.weight']))
    assert rel(db1, g['affine_unit_basic_stats.bias']) <= max(2e-6, 2 * rel(g32['affine_unit_basic_stats.bias'],
                                                                             g['affine_unit_basic_stats.bias']))
    for t, s in enumerate(TYPE_SUFFIX):
        want = g[f'affine_unit_{s}.weight']
        if want is None:
            assert dwt[t].abs().max().item() == 0.0
            continue
        assert rel(dwt[t], want) <= max(2e-6, 2 * rel(g32[f'affine_unit_{s}.weight'], want)), s


@pytest.mark.gpu
@pytest.mark.parametrize('algo,B', [('ppo', 8), ('vpg', 8), ('ppo', 16), ('ppo', 32)])
def test_exact_fused_step_deploy_shape_matches_fp64(gpu_ops, algo, B):
    """fp32-exact at B=8, S=1400: every gradient tensor within 1e-5 (relative) of float64 — the bf16x3 headline mode
    is pinned at 1e-3 (tests/test_fp32_kernels.py). The unit encoder's ∂W1 sits at ≈1.0-1.3e-5 for the plain torch-fp32
    evaluation itself under VPG and at B = 16 / 32 (the conditioning of that 11 200 × 8-row sum, not the kernels):
    there a tensor may reach 1.5× the torch-fp32 error instead (measured: fused 1.01e-5 vs torch 1.22e-5 VPG B=8,
    1.03e-5 vs 1.05e-5 PPO B=16, 1.09e-5 vs 1.26e-5 PPO B=32). B = 16 / 32: the exact recurrence with 2 / 4 rows per
    XCD chain (lstm_team.h: the Valu forms' rows)."""
    from tests.test_fp32_kernels import _rel, _step_grads
    (lf, _, gf), (lo, _, go), (l64, g64) = _step_grads('fp32-exact', 'lstm512', algo, B, 1400, fp64=True)
    rows = sorted(((_rel(gf[n], g64[n]), _rel(go[n], g64[n]), n) for n in g64
                   if g64[n] is not None and g64[n].norm() > 0), reverse=True)
    print(f'fp32-exact {algo} B={B}: worst (fused vs fp64, torch-fp32 vs fp64):', rows[:5], 'loss', lf, lo, l64)
    assert abs(lf - l64) <= 1e-6 * max(1e-2, abs(l64)), (lf, l64)
    bad = [r for r in rows if r[0] >= max(1e-5, 1.5 * r[1])]
    assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize('vbug', [False, True])
def test_exact_compat_network_matches_fp64(gpu_ops, vbug):
    """The reference's OWN network (compat preset: linear fake_rnn, the enemy-tower pool quirk, VPG, optionally the
    (B,S,S) value-target quirk — policy.py:67-68, 127, 143-145; optimizer.py:602-672) on the hand-written kernels
    (exact encoder → forward chain with the fake_rnn as its second product → heads GEMM → heads/loss kernel →
    ∂X chain → encoder backward, split-K weight gradients), deploy shape B=8, S=1400: every gradient tensor within
    1e-5 of float64 (or 1.5× the torch-fp32 error where that is larger)."""
    from dotaclient_amd.learner.engine import Learner, LossConfig
    from dotaclient_amd.learner.synthetic import make_batch
    from tests.test_fp32_kernels import _rel, _step_grads
    (lf, _, gf), (lo, _, go), (l64, g64) = _step_grads('fp32-exact', 'compat', 'vpg', 8, 1400, fp64=True, vbug=vbug)
    rows = sorted(((_rel(gf[n], g64[n]), _rel(go[n], g64[n]), n) for n in g64
                   if g64[n] is not None and g64[n].norm() > 0), reverse=True)
    print(f'compat vbug={vbug}: worst (fused vs fp64, torch-fp32 vs fp64):', rows[:5], 'loss', lf, lo, l64)
    assert abs(lf - l64) <= 1e-5 * max(1e-2, abs(l64)), (lf, l64)
    bad = [r for r in rows if r[0] >= max(1e-5, 1.5 * r[1])]
    assert not bad, bad[:5]
    # the direct (graph-capturable) step assembles the same loss on the device (norms[6:8] from time-major rows)
    torch.manual_seed(0)
    cfg = get_config('compat')
    lc = LossConfig(algo='vpg', vf_coef=0.5, entropy_coef=0.01, compat_value_bug=vbug)
    L = Learner(Policy(cfg), lc, device='cuda', backend='fused', dp=False, precision='fp32-exact')
    assert L.direct()
    batch = make_batch(8, 1400, cfg.layout, None, device='cuda', seed=3)
    m = L.train_step(batch)
    torch.cuda.synchronize()
    assert abs(float(m['loss']) - l64) <= 1e-5 * max(1e-2, abs(l64)), (float(m['loss']), l64)


@pytest.mark.gpu
def test_exact_5v5_step_matches_fp64(gpu_ops):
    """The 5v5 entity-attention learner at fp32-exact (BASELINE config 4 at the reference precision) on the IEEE-fp32
    twins of the attention block kernels (ops/csrc/attn_block.hip EX = true), the exact encoder backward with the
    block's ∂E0 as its input, exact ∂W_qkv / ∂W_out GEMMs — deploy shape B=8, S=1400: every gradient tensor within
    1e-5 of float64, or 1.5× the torch-fp32 error where that is larger."""
    from tests.test_fp32_kernels import _rel, _step_grads
    (lf, _, gf), (lo, _, go), (l64, g64) = _step_grads('fp32-exact', '5v5', 'ppo', 8, 1400, fp64=True)
    rows = sorted(((_rel(gf[n], g64[n]), _rel(go[n], g64[n]), n) for n in g64
                   if g64[n] is not None and g64[n].norm() > 0), reverse=True)
    print('5v5 fp32-exact: worst (fused vs fp64, torch-fp32 vs fp64):', rows[:6], 'loss', lf, lo, l64)
    assert abs(lf - l64) <= 1e-6 * max(1e-2, abs(l64)), (lf, l64)
    bad = [r for r in rows if r[0] >= max(1e-5, 1.5 * r[1])]
    assert not bad, bad[:5]

