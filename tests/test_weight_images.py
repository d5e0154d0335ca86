"""The fused step's weight operands (models/pipelined.py ``WeightImages``): every role equals the operand built directly
from the module's parameters, at both precisions; the gather kernel reproduces the index maps bit for bit; and the step
reads everything it gathers."""
import dataclasses

import pytest
import torch

from dotaclient_amd.models.pipelined import WeightImages, _frag_order, _k16_order
from dotaclient_amd.models.policy import TYPE_SUFFIX, Policy, get_config
from dotaclient_amd.ops.lstm import gate_perm
from dotaclient_amd.parallel.dp import FlatParams

PRECISIONS = ['fp32', 'fp32-exact']


# ---- the oracle: what one ``weight_prep`` launch computes from the maps ----------------------------------------------
def _take(flat, m):
    m = m.long()
    return torch.where(m >= 0, flat[m.clamp_min(0)], torch.zeros((), dtype=flat.dtype))


def _split(v):
    """hi = bf16(v), lo = bf16(v − float(hi)): round-to-nearest-even, like the kernel's f2bf."""
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def _oracle(wi, flat):
    """(buf32, bufH, bufL) of ``wi``'s maps applied to ``flat`` (CPU tensors)."""
    m32 = wi.map32.cpu().view(-1, 2)
    b32 = _take(flat, m32[:, 0]) + _take(flat, m32[:, 1])
    if wi.mapS is None:
        return b32, None, None
    return (b32,) + _split(_take(flat, wi.mapS.cpu()))


def _refresh_on_cpu(wi):
    b32, bh, bl = _oracle(wi, wi.flat)
    wi.buf32.copy_(b32)
    if bh is not None:
        wi.bufH.copy_(bh)
        wi.bufL.copy_(bl)
    return wi.views


# ---- the operands, built directly from the module's parameters ---------------------------------------------------------
def _slab(w):
    R, K = w.shape
    return w.reshape(R, K // 32, 32).permute(1, 0, 2).contiguous()


def _expected(pol, precision, with_value):
    cfg = pol.config
    P = {n: p.detach() for n, p in pol.named_parameters()}
    H = cfg.hidden
    lstm = cfg.rnn == 'lstm'
    exact = precision == 'fp32-exact'
    empty = torch.empty(0)

    def operand(w, order=None):
        w = w.contiguous()
        if exact:       # the fp32 matrix as it is (attention: in fragment order) and an empty lo
            return (order(w) if order else w), empty
        return tuple((order or _slab)(t) for t in _split(w))

    wt = torch.stack([P[f'affine_unit_{s}.weight'] for s in TYPE_SUFFIX])
    bt = torch.stack([P[f'affine_unit_{s}.bias'] for s in TYPE_SUFFIX])
    wpre = P['affine_pre_rnn.weight']
    if lstm:
        perm = gate_perm(H, 'cpu')
        w_in = P['rnn.weight_ih_l0'][perm]          # rows in unit-major gate order
        rec_b = (P['rnn.bias_ih_l0'] + P['rnn.bias_hh_l0'])[perm]
    else:
        w_in, rec_b = P['fake_rnn.weight'], P['fake_rnn.bias']
    heads = ('affine_unit_attention', 'affine_head_enum', 'affine_move_x', 'affine_move_y')
    wv = P['affine_value.weight'] if with_value else torch.zeros(1, H)
    bv = P['affine_value.bias'] if with_value else torch.zeros(1)
    wcat = torch.cat([P[f'{h}.weight'] for h in heads] + [wv, torch.zeros(256 - 150, H)], 0)
    bcat = torch.cat([P[f'{h}.bias'] for h in heads] + [bv, torch.zeros(256 - 150)])
    assert wcat.shape == (256, H)
    E = {'enc_w': wt, 'enc_wT': wt.transpose(1, 2).contiguous(), 'enc_b': bt,
         'pre_w': operand(wpre), 'pre_b': P['affine_pre_rnn.bias'], 'in_w': operand(w_in),
         'heads_w': operand(wcat), 'heads_b': bcat, 'heads_wT': operand(wcat.t()),
         'dx_in_wT': operand(w_in.t()), 'dx_pre_wT': operand(wpre.t()), 'rec_b': rec_b}
    if lstm:
        E['rec_w'] = P['rnn.weight_hh_l0']
    if cfg.entity_attention:
        wq, wo, bo = P['entity_attn.qkv.weight'], P['entity_attn.out.weight'], P['entity_attn.out.bias']
        E['enc_b'] = bt + bo[None]
        E['attn_out_b'] = bo
        E['attn_qkv_w'] = operand(wq, _frag_order)
        E['attn_out_w'] = operand(wo, _frag_order)
        E['attn_out_wT'] = operand(wo.t(), _frag_order)
        E['attn_qkv_k16'] = operand(wq, _k16_order)
    return E


def _policy(preset, seed=0, **over):
    cfg = dataclasses.replace(get_config(preset), **over)
    pol = Policy(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in pol.parameters():      # biases too: zero-initialised ones would hide a wrong bias source
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    return pol


def _images(pol, flat, precision, with_value):
    cfg = pol.config
    perm = gate_perm(cfg.hidden, 'cpu') if cfg.rnn == 'lstm' else None
    return WeightImages(cfg, pol.named_parameters(), flat, precision, with_value, perm)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('preset,with_value', [('lstm128', True), ('compat', True), ('5v5', True), ('lstm128', False)])
def test_every_role_is_the_operand_built_from_the_parameters(preset, with_value, precision):
    pol = _policy(preset)
    fl = FlatParams(pol)
    wi = _images(pol, fl.flat, precision, with_value)
    got = _refresh_on_cpu(wi)
    want = _expected(pol, precision, with_value)
    assert set(got) == set(want)
    for role, w in want.items():
        if isinstance(w, tuple):
            assert isinstance(got[role], tuple) and len(got[role]) == 2, role
            assert _same(got[role][0], w[0]) and _same(got[role][1], w[1]), role
        else:
            assert _same(got[role], w), role
    if precision == 'fp32-exact':
        assert wi.mapS is None
        los = {got[r][1].data_ptr() for r, w in want.items() if isinstance(w, tuple)}
        assert len(los) == 1                     # one empty lo, made once
    else:
        # the bf16x3 operands are gathered as hi / lo images only: no fp32 copy of them beside
        assert wi.buf32.numel() == sum(w.numel() for w in want.values() if not isinstance(w, tuple))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_uncovered_hidden_size_raises_with_the_dimension(precision):
    pol = _policy('lstm128', hidden=192)
    fl = FlatParams(pol)
    with pytest.raises(ValueError, match='192'):
        _images(pol, fl.flat, precision, True)


# ---- on the GPU ------------------------------------------------------------------------------------------------------
def _learner(preset, precision):
    from dotaclient_amd.learner.engine import Learner, LossConfig
    torch.manual_seed(0)
    lc = LossConfig(algo='vpg' if preset == 'compat' else 'ppo', vf_coef=0.5, entropy_coef=0.01)
    return Learner(_policy(preset), lc, device='cuda', backend='fused', dp=False, precision=precision)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('preset', ['lstm128', '5v5'])
def test_refresh_is_bitwise_the_oracle(gpu_ops, preset, precision):
    L = _learner(preset, precision)
    wi = L.model.weight_images()
    wi.refresh(gpu_ops)
    torch.cuda.synchronize()
    b32, bh, bl = _oracle(wi, wi.flat.cpu())
    assert torch.equal(wi.buf32.cpu().view(torch.int32), b32.view(torch.int32))
    assert (bh is None) == (precision == 'fp32-exact')
    if bh is not None:
        assert torch.equal(wi.bufH.cpu().view(torch.int16), bh.view(torch.int16))
        assert torch.equal(wi.bufL.cpu().view(torch.int16), bl.view(torch.int16))


class _Reads(dict):
    """The role → operand mapping, recording which roles are read."""

    def __init__(self, d):
        super().__init__(d)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('preset,B,S', [('lstm128', 2, 24), ('compat', 2, 24), ('5v5', 1, 16)])
def test_the_step_reads_every_gathered_role(gpu_ops, preset, B, S, precision):
    from dotaclient_amd.learner.synthetic import make_batch
    L = _learner(preset, precision)
    cfg = L.model.cfg
    batch = make_batch(B, S, cfg.layout, cfg.hidden if cfg.rnn == 'lstm' else None, device='cuda', seed=3)
    rows, B_, S_ = L.batch_to_time_major(batch)
    wi = L.model.weight_images()
    gathered = set(wi.views)
    wi.views = rec = _Reads(wi.views)
    vec = L._direct_body(rows, B_, S_)
    torch.cuda.synchronize()
    assert L.model.weight_images() is wi
    assert bool(torch.isfinite(vec[0]))
    assert rec.read == gathered, sorted(gathered - rec.read)
    rec.read = set()
    lp, v = L.model.forward_logp_value(rows, B_, S_)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lp).all())
    assert rec.read and rec.read < gathered     # the forward half reads a subset
