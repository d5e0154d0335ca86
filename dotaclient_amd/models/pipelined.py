"""The fused LSTM learner step: time-major core, weight images, and the autograd-free direct step.

Rows are processed TIME-MAJOR (row = t·B + b): a time step is a contiguous slice of every activation. The loss
and every gradient are computed in ONE pass of explicit kernels (no autograd graph) — :func:`fused_step_tm` =
:func:`_forward` → :func:`_heads_loss` → :func:`_backward`, over two streams (the recurrences and, behind them, most
weight-gradient GEMMs on the side stream; everything else on the main stream); two ways in:

* :class:`PipelinedPolicyLoss` — an ``autograd.Function`` over batch-major inputs (transposed once on entry) whose
  ``backward`` only scales the precomputed gradients by the upstream gradient (used by ``Learner.loss`` callers
  that backprop themselves, and by tests);
* :func:`train_direct` — the learner's hot path: time-major inputs (gathered straight from the HBM replay,
  ``learner.engine.Learner.train_step_replay``), loss normalisers from one kernel (``loss_prep``), the weight
  operands the step reads at its precision from one gather kernel (``weight_prep``, :class:`WeightImages`, which
  alone decides each operand's form: the step passes ``W[role]`` on as it is), gradients written
  into the flat gradient buffer by one multi-tensor kernel and the loss + metrics by one kernel
  (``loss_assemble``) — about 120 fewer launches per step than the autograd route, and the whole step is
  capturable in one hipGraph.

The step runs over the whole sequence at once. Splitting it into time chunks, software-pipelined over the two
streams (each chunk's heads and weight gradients beside the next chunk's recurrence), was built and measured twice on
MI355X and removed: work on the other XCDs slows the L2-bound recurrence more than the overlap saves (5.78 ms whole
against 6.24 / 6.98 ms at 2 / 4 chunks, profiles/r4_chunk_overlap_probe.md; 5.45 ms against 6.2-6.9 ms, the
CU-exclusive half teams built for it included, profiles/r5_half_team.md).

Precisions: ``fp32-exact`` (IEEE fp32 products) and ``fp32`` (fp32 activations, bf16x3-split MFMA operands). Every
product of the step runs in a hand-written kernel — there is no vendor-GEMM branch; a bf16 learner runs on the torch
backend (learner/engine.py).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch

from ..ops.lstm import team_bwd, team_fwd, team_plan
from .policy import TYPE_SUFFIX

LDZ = 160

# parameters whose gradient the direct step accumulates in place (split-K GEMM straight into the flat grad buffer)
DIRECT_GEMM_GRADS = ('rnn.weight_hh_l0', 'rnn.weight_ih_l0', 'affine_pre_rnn.weight', 'affine_pre_rnn.bias')

METRIC_NAMES = ['loss', 'policy_loss', 'entropy_loss', 'advantage_loss', 'entropy', 'advantage', 'approx_kl',
                'clipfrac', 'entropy/enum', 'entropy/x', 'entropy/y', 'entropy/target_unit',
                # in-step V-trace (LossConfig.vtrace): mean truncated importance weight, fraction truncated, and the
                # behaviour KL estimate mean(log μ − log π) of the minibatch
                'offpolicy/rho_mean', 'offpolicy/rho_truncated', 'offpolicy/behaviour_kl']


def _frag_order(w: torch.Tensor) -> torch.Tensor:
    """(R, K) bf16 → MFMA fragment order [R/16][K/32][lane = 16·(k%32 // 8) + r%16][8] (ops/csrc/attn_block.hip)."""
    R, K = w.shape
    return w.view(R // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def _k16_order(w: torch.Tensor) -> torch.Tensor:
    """(R, K) bf16 → 16x16x16 B-fragment order [R/16][K/16][lane = 16·(r%16 // 4) + k%16][4]: element j of lane l is
    w[16·rt + 4·(l>>4) + j][16·ct + (l&15)] (ops/csrc/attn_block.hip gfrag4)."""
    R, K = w.shape
    return w.view(R // 16, 4, 4, K // 16, 16).permute(0, 3, 1, 4, 2).contiguous()


def _slab_major(w: torch.Tensor) -> torch.Tensor:
    """(R, K) → slab-major [K/32][R][32]: a wave's weight load of the chain kernels is 1 KB contiguous
    (ops/csrc/dx_chain.hip)."""
    R, K = w.shape
    return w.reshape(R, K // 32, 32).permute(1, 0, 2).contiguous()


# Forms of a weight operand. F32: fp32 gather; SUM: fp32 sum of two sources. The MFMA weight operands are (hi, lo)
# pairs in the order their kernel loads them — bf16 hi / lo images (x = hi + lo) at fp32, the fp32 image and an empty
# lo at fp32-exact: MAT a matrix of the chain kernels (slab-major hi / lo, or the fp32 matrix as it is), FRAG / K16 the
# attention block's fragment orders (the same order at both precisions).
F32, SUM, MAT, FRAG, K16 = 'f32', 'sum', 'mat', 'frag', 'k16'
# form → (image order of the hi / lo pair, image order of the exact fp32 operand)
_ORDER = {MAT: (_slab_major, torch.Tensor.contiguous), FRAG: (_frag_order, _frag_order), K16: (_k16_order, _k16_order)}


def _operand_table(cfg, idx, perm, with_value: bool):
    """(role, source index expression, form) of every weight operand the fused step reads. ``idx(name)``: the flat
    buffer indices of a parameter, in its shape; −1 = a zero. Roles are named for what they feed."""
    H = cfg.hidden
    lstm = cfg.rnn == 'lstm'
    neg = lambda *shape: torch.full(shape, -1, dtype=torch.int64)  # noqa: E731
    wt = torch.stack([idx(f'affine_unit_{s}.weight') for s in TYPE_SUFFIX])
    bt = torch.stack([idx(f'affine_unit_{s}.bias') for s in TYPE_SUFFIX])
    wpre = idx('affine_pre_rnn.weight')
    # the recurrent layer's input weight: W_ih (rows in unit-major gate order) or the reference's linear fake_rnn W_f
    # (policy.py:67-68, 143-145)
    w_in = idx('rnn.weight_ih_l0')[perm] if lstm else idx('fake_rnn.weight')
    # W_cat = [attention | enum | x | y | value | 0-pad], zero-padded to the 256 rows of the chain kernel's stage
    heads = ('affine_unit_attention', 'affine_head_enum', 'affine_move_x', 'affine_move_y')
    wv, bv = (idx('affine_value.weight'), idx('affine_value.bias')) if with_value else (neg(1, H), neg(1))
    wcat = torch.cat([idx(f'{h}.weight') for h in heads] + [wv, neg(256 - 150, H)], 0)
    bcat = torch.cat([idx(f'{h}.bias') for h in heads] + [bv, neg(256 - 150)])
    enc_b = ('enc_b', bt, F32)
    if cfg.entity_attention:
        # 5v5: the encoder adds b_τ + b_out (E0' = E0 + b_out; LayerNorm subtracts it again and the out-projection
        # then accumulates onto E0' in place: no residual copy, no bias pass)
        wq, wo, bo = idx('entity_attn.qkv.weight'), idx('entity_attn.out.weight'), idx('entity_attn.out.bias')
        enc_b = ('enc_b', (bt, bo.unsqueeze(0).expand(6, -1)), SUM)
    rows = [
        ('enc_w', wt, F32),                             # encoder: (6, 128, 128) type weights
        ('enc_wT', wt.transpose(1, 2), F32),            # encoder backward: their transposes
        enc_b,                                          # (6, 128)
        ('pre_w', wpre, MAT),                           # forward chain: W_pre (256, 896)
        ('pre_b', idx('affine_pre_rnn.bias'), F32),
        ('in_w', w_in, MAT),                            # forward chain: W_ih (4H, 256) / W_f (H, 256)
        ('heads_w', wcat, MAT),                         # heads GEMM: W_cat (256, H)
        ('heads_b', bcat, F32),
        ('heads_wT', wcat.t(), MAT),                    # ∂h = ∂z·W_cat
        ('dx_in_wT', w_in.t(), MAT),                    # ∂X chain: ∂pre = ∂G·W_ih, K-contiguous per column
        ('dx_pre_wT', wpre.t(), MAT),                   # ∂X chain: ∂x896 = ∂pre·W_pre
    ]
    if lstm:
        rows += [('rec_w', idx('rnn.weight_hh_l0'), F32),      # recurrence: W_hh (4H, H), PyTorch's row order
                 ('rec_b', (idx('rnn.bias_ih_l0')[perm], idx('rnn.bias_hh_l0')[perm]), SUM)]   # unit-major (4H)
    else:
        rows += [('rec_b', idx('fake_rnn.bias'), F32)]
    if cfg.entity_attention:
        rows += [('attn_out_b', bo, F32),
                 ('attn_qkv_w', wq, FRAG), ('attn_out_w', wo, FRAG),            # attention block forward
                 ('attn_out_wT', wo.t().contiguous(), FRAG), ('attn_qkv_k16', wq, K16)]   # and backward
    return rows


class WeightImages:
    """Per-step working copies of the weights, produced by ONE ``weight_prep`` gather launch from the flat fp32
    parameter buffer (instead of ≈25 cast / stack / permute / cat launches), and the only place that knows which form
    a kernel's weight operand takes at ``precision`` ('fp32' = bf16x3, 'fp32-exact'): :func:`_operand_table` names the
    operands, :meth:`refresh` returns role → fp32 tensor, or → the ready (hi, lo) argument pair of an MFMA operand.
    Only what the step reads at that precision is gathered. The index maps are built once, from the parameters' offsets
    in the flat buffer; ``perm``: the gate permutation (ops/lstm.py ``gate_perm``, on the CPU) of an LSTM policy."""

    def __init__(self, cfg, named_params, flat: torch.Tensor, precision: str, with_value: bool,
                 perm: Optional[torch.Tensor] = None):
        if precision not in ('fp32', 'fp32-exact'):
            raise ValueError(f'the fused step runs at fp32 / fp32-exact, not {precision!r}')
        exact = precision == 'fp32-exact'
        dev = flat.device
        base = flat.data_ptr()
        P = dict(named_params)

        def idx(name):
            p = P[name]
            assert p.is_contiguous() and p.dtype == torch.float32
            off = (p.data_ptr() - base) // 4
            assert 0 <= off and off + p.numel() <= flat.numel(), f'{name} is not a view of the flat buffer'
            return torch.arange(p.numel(), dtype=torch.int64).view(p.shape) + off

        # role → (…, 2) source pairs of an fp32 image / → sources of a hi / lo image; the MFMA operands' roles
        gather, split, operands = {}, {}, set()
        for role, src, form in _operand_table(cfg, idx, perm, with_value):
            if form == MAT and any(d % 128 for d in src.shape):
                raise ValueError(f'WeightImages: {role} is {tuple(src.shape)}; the kernels cover multiples of 128 '
                                 f'(hidden {cfg.hidden}, pre-RNN width {cfg.pre_rnn_dim})')
            if form in _ORDER:
                operands.add(role)
                src = _ORDER[form][exact](src)
                if not exact:
                    split[role] = src
                    continue
            a, b = src if form == SUM else (src, torch.full_like(src, -1))
            gather[role] = torch.stack([a, b], -1)      # (stack copies the broadcast view of a shared second term)
        self.flat = flat
        self.map32 = torch.cat([m.reshape(-1, 2) for m in gather.values()]).to(torch.int32).to(dev)
        self.buf32 = torch.empty(self.map32.shape[0], dtype=torch.float32, device=dev)
        self.mapS = self.bufH = self.bufL = None
        if split:
            self.mapS = torch.cat([m.reshape(-1) for m in split.values()]).to(torch.int32).to(dev)
            self.bufH = torch.empty(self.mapS.numel(), dtype=torch.bfloat16, device=dev)
            self.bufL = torch.empty_like(self.bufH)
        no_lo = torch.empty(0, dtype=torch.float32, device=dev)     # the lo slot of every fp32-exact operand
        self.views: Dict[str, object] = {}
        o = 0
        for role, m in gather.items():
            v = self.buf32[o:o + m[..., 0].numel()].view(m.shape[:-1])
            self.views[role] = (v, no_lo) if role in operands else v
            o += v.numel()
        o = 0
        for role, m in split.items():
            self.views[role] = (self.bufH[o:o + m.numel()].view(m.shape), self.bufL[o:o + m.numel()].view(m.shape))
            o += m.numel()

    def refresh(self, C) -> Dict[str, object]:
        C.weight_prep(self.flat, self.map32, self.buf32, self.mapS, self.bufH, self.bufL)
        return self.views


# Fixed choices of the step, each measured against its alternative in earlier rounds (the alternatives were removed):
# * the weight-gradient GEMMs of the recurrence and pre-RNN layer run on the (then idle) recurrence stream, beside the
#   ∂X chain of the main stream; in the exact learner ∂W_pre / ∂b_pre go to the main stream after the encoder
#   backward instead (5.514 vs 5.560 ms per step; the bf16x3 learner keeps them on the side stream: 4.911 vs 4.921);
# * the fp32 forward chain relu(x896·W_preᵀ + b)·W_ihᵀ, the heads GEMM and its ∂X product, and the ∂X chain
#   (∂G·W_ih)⊙[x>0]·W_pre are hand-written kernels (ops/csrc/dx_chain.hip), not vendor GEMMs;
# * the fp32 5v5 attention block forward and backward are one kernel each (ops/csrc/attn_block.hip; the five-launch
#   backward took 1858 vs 1660 µs); fp32-exact runs their IEEE-fp32 twins (the same kernels templated on the operand
#   precision); ∂W_out on the main stream after the encoder backward, ∂W_qkv alone on the side stream (both GEMMs
#   serial on the side stream left ∂W_qkv exposed at the step's end, profiles/r5_5v5_exact_timeline.txt; a third
#   stream for ∂W_out measured 0.27 ms slower, profiles/r6_gemm_map_and_5v5_streams.md);
# * the exact recurrence's gate activations use the hardware exp / reciprocal: products-exact, the same worst
#   tensor errors against float64 as libm expf / tanhf (PPO 2.50e-6 both), 0.5 ms per step faster.


class Forward(NamedTuple):
    """What :func:`_forward` saves for the heads / loss and the backward, time-major rows."""
    x896: torch.Tensor                    # (N, 896) encoder output: env | own hero | five type pools
    emb: torch.Tensor                     # (N, U, 128) unit embeddings (5v5: after the attention block)
    arg: torch.Tensor                     # (N, 6, 128) u8 argmax of the type pools
    x16: torch.Tensor                     # (N, 256) relu(pre-RNN)
    hs: torch.Tensor                      # (S, B, H) recurrence output
    cs: Optional[torch.Tensor]            # (S, B, H) cell states (None: linear fake_rnn)
    gates4: Optional[torch.Tensor]        # (S, B, H, 4) activated gates (None: linear fake_rnn)
    z: torch.Tensor                       # (N, 256) heads GEMM: pointer query | enum | x | y | value | 0-pad
    attn: Optional[tuple]                 # 5v5: (E0', Xn, ln_mu, ln_rs, QKV, Oat, lse) of the attention block


class Heads(NamedTuple):
    """What :func:`_heads_loss` returns."""
    part: torch.Tensor                    # (R, 16) loss partials
    logp: torch.Tensor                    # (N,) log-prob of the taken actions
    dz: torch.Tensor                      # (N, 256) ∂L/∂z
    dtl: torch.Tensor                     # (N, U) ∂L/∂pointer logits
    dxh: torch.Tensor                     # (S, B, H) ∂L/∂h from the heads


def _forward(fp, W: Dict[str, torch.Tensor], P: Dict[str, torch.Tensor], units_t, env_t, h0, c0, B: int, S: int,
             rst: Optional[torch.Tensor]) -> Forward:
    """Encoder [+ attention block] → forward chain → recurrence (on the side stream) → heads GEMM. On return the
    current stream has joined the side stream."""
    C, cfg = fp.C, fp.cfg
    exact = fp.exact
    lin = cfg.rnn != 'lstm'             # the reference's linear fake_rnn layer (compat preset): no recurrence
    N, U, H = B * S, units_t.shape[1], cfg.hidden
    dev = units_t.device
    main = torch.cuda.current_stream(dev)
    sL = fp.side_stream()
    w1, b1 = P['affine_unit_basic_stats.weight'].detach(), P['affine_unit_basic_stats.bias'].detach()
    we, be = P['affine_env.weight'].detach(), P['affine_env.bias'].detach()
    # (exact: the IEEE-fp32 encoder variant, ops/csrc/encoder.hip encoder_fwd_x_kernel)
    x896, emb, arg = C.encoder_fwd(units_t, env_t, w1, b1, W['enc_w'], W['enc_b'], we, be, list(cfg.layout.counts),
                                   bool(cfg.compat_bugs), exact=exact)
    attn = None
    if cfg.entity_attention:
        # 5v5 entity attention, ONE kernel (ops/csrc/attn_block.hip attn_block_fwd_f32_kernel): LayerNorm → QKV
        # (bias added in the kernel) → 4-head self-attention → out-projection onto E0' = E0 + b_out (bias folded into
        # bt) → pools / argmax of the attended embeddings; bf16x3 operands (hi / lo fragment images), or the IEEE-fp32
        # twin on fp32 fragment images at fp32-exact. E0' stays untouched (the LayerNorm backward's input), E1 is new
        E0p = emb.view(N * U, 128)
        arg = torch.empty(N, 6, 128, dtype=torch.uint8, device=dev)
        Xn, ln_mu, ln_rs, QKV, Oat, lse, E1 = C.attn_block_fwd(
            E0p, W['attn_out_b'], P['entity_attn.ln.weight'].detach(), P['entity_attn.ln.bias'].detach(),
            *W['attn_qkv_w'], P['entity_attn.qkv.bias'].detach(), *W['attn_out_w'], fp.type_offset_list(), x896, arg,
            bool(cfg.compat_bugs), 1e-5)
        emb = E1.view(N, U, 128)
        attn = (E0p, Xn, ln_mu, ln_rs, QKV, Oat, lse)
    elif cfg.compat_bugs:   # reference policy.py:127: enemy-tower pool = enemy-nonhero pool
        x896[:, 768:896] = x896[:, 512:640]
        arg[:, 5] = arg[:, 3]
    # the forward chain relu(x896·W_preᵀ + b)·W_ihᵀ in ONE kernel (ops/csrc/dx_chain.hip; x16 > 0 ⟺ x > 0): slab-major
    # bf16 hi / lo weight images, or the fp32 weights as they are on v_mfma_f32_16x16x4_f32
    x16, xp = C.pre_rnn_chain(x896, *W['pre_w'], W['pre_b'], *W['in_w'])
    if lin:
        # fake_rnn: h = pre·W_fᵀ + b_f (the chain kernel's second product) — no activation, no recurrence
        hs = xp.add_(W['rec_b']).view(S, B, H)
        cs = gates4 = None
    else:
        hs = torch.empty(S, B, H, device=dev)
        cs = torch.empty(S, B, H, device=dev)
        gates4 = torch.empty(S, B, H, 4, device=dev)
    sL.wait_stream(main)
    if not lin:
        with torch.cuda.stream(sL):
            team_fwd(C, xp.view(S, B, H, 4), W['rec_w'], h0, c0, fp.err, False, time_major=True, hs_out=hs,
                     cs_out=cs, gates_out=gates4, bias4=W['rec_b'], reset=rst, exact=exact)
        main.wait_stream(sL)
    # heads GEMM on the chain kernel's stages (bf16x3 images, or exact: fp32 W_cat padded to 256 rows)
    z = C.rowmm_out256(hs.view(N, H), *W['heads_w'], W['heads_b'])   # (N, 256), padding columns 0
    return Forward(x896, emb, arg, x16, hs, cs, gates4, z, attn)


def _heads_loss(fp, W: Dict[str, torch.Tensor], f: Forward, act_t, msk_t, adv_t, ret_t, lpo_t, nret_t, norms,
                B: int, S: int, vt_t: Optional[torch.Tensor]) -> Heads:
    """The heads / loss kernel (loss partials, log-probs, ∂z, ∂pointer logits) and ∂h = ∂z·W_cat, preceded by the
    in-step V-trace when ``vt_t`` is given. Sets ``fp.vtrace_stats``. ``fp.seq_weight`` ((B,) f32 at a fixed address:
    the importance weights of a prioritised replay's sampling pass, learner/engine.py) weights the sequences' loss
    terms in the loss call; the forward-only V-trace call and the priorities never see it."""
    C, lc = fp.C, fp.loss_cfg
    exact = fp.exact
    N, H = B * S, fp.cfg.hidden
    # heads_loss algo: 0 = PPO clipped surrogate, 1 = VPG (reference), 2 = PPO's truncated-IS off-policy term
    algo = (2 if getattr(lc, 'offpolicy', 'clip') == 'tis' else 0) if lc.algo == 'ppo' else 1
    fp.vtrace_stats = None
    sw = getattr(fp, 'seq_weight', None)
    if sw is not None and (algo == 1 or sw.numel() != B):
        raise ValueError('per-sequence loss weights: one weight per sequence, PPO objectives only (not the VPG loss)')
    if vt_t is not None:
        # V-trace INSIDE the step (LossConfig.vtrace): this step's own values (z column 149) and log-probs of the
        # recorded actions (a first, forward-only pass of the heads kernel) against the actor's behaviour
        # log-probs (lpo_t) give the advantages and value targets — for fresh and replayed experience alike,
        # at the weights being trained (ops/csrc/scan.hip vtrace_step_kernel), then normalised over the valid rows
        from ..constants import EPS
        from ..ops.scan import vtrace_step
        zero = fp.scratch('vt_zero', (N,), torch.float32, f.z.device)
        _, _, _, lp_a = C.heads_loss(f.z, f.emb, act_t, msk_t, zero, zero, zero, zero, norms, 0, False, S, B,
                                     float(lc.clip_eps), 0.0, 0.0, dz_bf16=False, precise=exact)
        adv_v, ret_t, fp.vtrace_stats = vtrace_step(None, lp_a, lpo_t, vt_t, B, S, lc.gamma, lc.gae_lambda,
                                                    getattr(lc, 'vtrace_rho_bar', 1.0),
                                                    getattr(lc, 'vtrace_c_bar', 1.0), z=f.z, vcol=149)
        pc = getattr(fp, 'priority_cfg', None)
        if pc is not None:
            # the step trains from a prioritised replay (learner/engine.py): the sequences' new priorities from the
            # un-normalised advantages, into the policy's persistent (2, B) buffer (ops/csrc/replay_sample.hip)
            from ..ops.replay import seq_priority
            seq_priority(adv_v, vt_t.contiguous(), fp.scratch(f'seq_priority_{B}', (2, B), torch.float32, f.z.device), B, S, *pc)
        adv_t = torch.empty_like(adv_v)
        C.adv_normalize(adv_v, vt_t[:, 2].contiguous(), adv_t, float(EPS))
    dz, dtl, part, logp = C.heads_loss(f.z, f.emb, act_t, msk_t, adv_t, ret_t, lpo_t, nret_t, norms, algo,
                                       bool(lc.compat_value_bug), S, B, float(lc.clip_eps), float(lc.entropy_coef),
                                       float(lc.vf_coef), dz_bf16=False, precise=exact, seq_weight=sw)
    dxh = C.rowmm_in256(dz, *W['heads_wT']).view(S, B, H)
    return Heads(part, logp, dz, dtl, dxh)


def _backward(fp, W: Dict[str, torch.Tensor], P: Dict[str, torch.Tensor], f: Forward, hd: Heads, units_t, env_t,
              h0, c0, B: int, S: int, gout: Optional[Dict[str, torch.Tensor]], rst: Optional[torch.Tensor],
              heads_done: torch.cuda.Event) -> Dict[str, torch.Tensor]:
    """Every parameter gradient. The side stream runs the backward recurrence and then, idle, the weight-gradient
    GEMMs of the heads, W_hh, W_ih and the pre-RNN layer, off the critical ∂X chain (∂pre → ∂x896 → [attention
    backward →] encoder backward) of the main stream; the main stream joins it before the DP split point and before
    returning. ``heads_done``: recorded on the main stream after :func:`_heads_loss`."""
    from ..ops.gemm import gemm_tn as _gemm_tn
    C, cfg = fp.C, fp.cfg
    exact = fp.exact
    lin = cfg.rnn != 'lstm'
    attn = cfg.entity_attention
    N, H = B * S, cfg.hidden
    dev = units_t.device
    main = torch.cuda.current_stream(dev)
    sL = fp.side_stream()
    counts = list(cfg.layout.counts)
    w1, b1 = P['affine_unit_basic_stats.weight'].detach(), P['affine_unit_basic_stats.bias'].detach()
    we, be = P['affine_env.weight'].detach(), P['affine_env.bias'].detach()

    def gemm_tn(*a, **k):
        # weight gradients: split-K MFMA over the B·S rows (ops/csrc/gemm_tn.hip), written in PyTorch's gate-major row
        # order through the gate permutation; IEEE-fp32 learner: exact v_mfma_f32_16x16x4_f32
        return _gemm_tn(*a, exact=exact, **k)
    grads: Dict[str, torch.Tensor] = {}
    dbcat = torch.empty(LDZ, device=dev)
    dWcat = torch.empty(LDZ, H, device=dev)
    fp.split_head_grads(dWcat, dbcat, grads)
    # data-parallel split (direct mode): see the split point below
    direct = gout is not None
    split = fp.split_hook if direct else None
    early_names = fp.early_param_names() if split is not None else frozenset()
    fp.early_applied = frozenset()
    dgates = None if lin else torch.empty(S, B, H, 4, device=dev)   # ∂gates straight from the kernel
    if attn:
        dWout, dbout = torch.empty(128, 128, device=dev), torch.empty(128, device=dev)
        dWqkv, dbqkv = torch.empty(384, 128, device=dev), torch.empty(384, device=dev)
    gperm = fp.gate_perm_i32(H, dev)
    # in direct mode the big weight gradients are accumulated straight into the flat gradient buffer
    if lin:
        dWih = grads['fake_rnn.weight'] = torch.empty(H, f.x16.shape[1], device=dev)
        dbf = grads['fake_rnn.bias'] = torch.empty(H, device=dev)
    else:
        dWhh = gout['rnn.weight_hh_l0'] if direct else torch.zeros(4 * H, H, device=dev)
        dWih = gout['rnn.weight_ih_l0'] if direct else torch.zeros(4 * H, f.x16.shape[1], device=dev)
    dWpre = gout['affine_pre_rnn.weight'] if direct else torch.zeros_like(P['affine_pre_rnn.weight'])
    dbpre = gout['affine_pre_rnn.bias'] if direct else torch.zeros_like(P['affine_pre_rnn.bias'])
    sL.wait_event(heads_done)
    db = None
    with torch.cuda.stream(sL):
        if not lin:
            db = team_bwd(C, hd.dxh, f.gates4, f.cs, c0, None, None, W['rec_w'], fp.err, time_major=True,
                          dg_out=dgates, dg_bf16=False, want_dbias=True, reset=rst, exact=exact)[3]
            bwd_done = torch.cuda.Event()
            bwd_done.record(sL)
        # the heads' weight gradient waits behind the backward recurrence (off the path between the two recurrences)
        gemm_tn(hd.dz[:, :LDZ], f.hs.view(N, H), out=dWcat, colsum=dbcat)   # (the heads' columns of the 256-wide ∂z)
    if not lin:
        main.wait_event(bwd_done)
    dG = hd.dxh.view(N, H) if lin else dgates.view(N, 4 * H)
    with torch.cuda.stream(sL):
        if lin:
            gemm_tn(dG, f.x16, out=dWih, colsum=dbf)      # ∂W_f, ∂b_f (no recurrent weight)
        else:
            if rst is not None:
                # packed: the h_{t-1} operand is zero where an episode starts at t (the forward never used it)
                hprev = torch.cat([h0.unsqueeze(0), f.hs[:S - 1]], 0).masked_fill_(rst.bool().unsqueeze(2), 0.0)
                gemm_tn(dG, hprev.view(N, H), out=dWhh, perm=gperm, accumulate=True)
            else:       # h_{t-1} rows: h0 for t = 0, then hs[0 : S-1] — no concatenation materialised
                gemm_tn(dG, f.hs[0:S - 1].view(N - B, H), out=dWhh, perm=gperm, accumulate=True, b0=h0)
            gemm_tn(dG, f.x16, out=dWih, perm=gperm, accumulate=True)
    # ∂pre = (∂G·W_ih)⊙[x16 > 0] and ∂x896 = ∂pre·W_pre in one launch (the ∂pre tile stays in LDS); operands: bf16
    # hi / lo slab images, or the fp32 transposes as they are
    dpre, dx896 = C.dpre_dx(dG, *W['dx_in_wT'], f.x16, *W['dx_pre_wT'])

    def wpre_grad():
        gemm_tn(dpre, f.x896, out=dWpre, accumulate=True, colsum=dbpre)
    # ∂W_pre / ∂b_pre: exact learner without the DP split: on the main stream after the encoder backward (the side
    # stream ends with ∂W_ih); otherwise on the side stream, behind ∂W_ih
    pre_main = split is None and exact
    if not pre_main:
        sL.wait_stream(main)
        with torch.cuda.stream(sL):
            wpre_grad()
    if split is not None:
        main.wait_stream(sL)
        # DP split point: every gradient of the recurrence, pre-RNN and heads is final here (the big ones are
        # already in the flat buffer); apply the small ones and let the learner all-reduce those buckets while
        # the encoder backward below runs (see learner/graphs.py: the hook cuts the capture in two)
        if not lin:
            grads['rnn.bias_ih_l0'] = db         # (gate-major already: the kernel writes PyTorch's order)
            grads['rnn.bias_hh_l0'] = db
        early = [grads.pop(nm, None) if nm in early_names else None for nm in fp.param_names]
        fp.apply_direct_grads(early, None, set_mask=False)    # the final call records the full mask
        fp.early_applied = early_names
        split()
    demb_in = None
    if attn:
        # one kernel from ∂x896 / the pointer gradient to ∂E0
        E0p, Xn, ln_mu, ln_rs, QKV, Oat, lse = f.attn
        dE1, dQKV, demb_in, lnsum = C.attn_block_bwd(
            hd.dtl, f.z, dx896, f.arg, fp.type_offset_list(), bool(cfg.compat_bugs), Oat, QKV,
            P['entity_attn.qkv.bias'].detach(), lse, E0p, W['attn_out_b'], ln_mu, ln_rs,
            P['entity_attn.ln.weight'].detach(), *W['attn_out_wT'], *W['attn_qkv_k16'], None)

    def side_tail():
        with torch.cuda.stream(sL):
            if attn:
                # ∂W_qkv (the larger of the two weight gradients over the N·U unit rows: 384 × 128) alone on the side
                # stream from the attention backward on; ∂W_out goes to the main stream after the encoder backward — the
                # two streams' tails balance (profiles/r6_gemm_map_and_5v5_streams.md)
                gemm_tn(dQKV, Xn, out=dWqkv, colsum=dbqkv)
            # ∂b_τ, ∂W_env, ∂b_env: one pass over the rows (ops/csrc/glue.hip enc_small_grads), beside the encoder
            # backward
            return C.enc_small_grads(f.z, hd.dtl, fp.type_offsets(dev), dx896, env_t, we, be, bool(cfg.compat_bugs))
    # the side stream's tail waits on ∂x896 (5v5: on the attention backward), not on the encoder backward
    sL.wait_stream(main)
    if not attn:
        dbt, dWe, dbe = side_tail()
    dWt, dw1, db1 = C.encoder_bwd(units_t, w1, b1, W['enc_wT'], hd.dtl, f.z, dx896, f.arg, counts,
                                  bool(cfg.compat_bugs), demb_in=demb_in, exact=exact)
    if pre_main:
        wpre_grad()
    if attn:
        gemm_tn(dE1, Oat, out=dWout, colsum=dbout)
        # enqueued AFTER the encoder backward: issued before it, the graph ran the side stream's GEMM and then the
        # encoder backward strictly one after the other
        _, dWe, dbe = side_tail()
        dbt = lnsum[256:].view(6, 128)
    main.wait_stream(sL)
    if not direct:
        if not lin:
            grads['rnn.weight_hh_l0'] = dWhh
            grads['rnn.weight_ih_l0'] = dWih
        grads['affine_pre_rnn.weight'] = dWpre
        grads['affine_pre_rnn.bias'] = dbpre
    if not lin and 'rnn.bias_ih_l0' not in fp.early_applied:
        grads['rnn.bias_ih_l0'] = db
        grads['rnn.bias_hh_l0'] = db
    grads['affine_unit_basic_stats.weight'] = dw1
    grads['affine_unit_basic_stats.bias'] = db1
    for t, s in enumerate(TYPE_SUFFIX):
        grads[f'affine_unit_{s}.weight'] = dWt[t]
        grads[f'affine_unit_{s}.bias'] = dbt[t]
    grads['affine_env.weight'] = dWe
    grads['affine_env.bias'] = dbe
    if attn:
        grads['entity_attn.ln.weight'] = lnsum[:128]
        grads['entity_attn.ln.bias'] = lnsum[128:256]
        grads['entity_attn.qkv.weight'] = dWqkv
        grads['entity_attn.qkv.bias'] = dbqkv
        grads['entity_attn.out.weight'] = dWout
        grads['entity_attn.out.bias'] = dbout
    return grads


def fused_step_tm(fp, W: Dict[str, torch.Tensor], P: Dict[str, torch.Tensor], units_t, env_t, act_t, msk_t, adv_t,
                  ret_t, lpo_t, nret_t, norms, h0, c0, B: int, S: int, gout: Optional[Dict[str, torch.Tensor]] = None,
                  reset_t: Optional[torch.Tensor] = None, vt_t: Optional[torch.Tensor] = None):
    """Loss partials and all parameter gradients of one minibatch, from TIME-MAJOR rows (row = t·B + b): forward →
    heads / loss → backward, every product on a hand-written kernel (no torch GEMM, so no matmul mode to pin).

    ``W`` = :class:`WeightImages` operands by role, ``P`` = fp32 parameters (the small fp32 weights used directly).
    ``gout`` (direct mode): parameter name → gradient tensor (a view of the flat gradient buffer); the big
    weight-gradient GEMMs (W_hh, W_ih, pre-RNN) ACCUMULATE straight into those and are left out of ``grads``.
    Returns (partials (R,16) f32, logp (N) f32 time-major, grads {param name → tensor})."""
    assert fp.fp32, 'the fused step runs at fp32 / fp32-exact (bf16: torch backend)'
    if fp.exact and fp.cfg.rnn == 'lstm':
        # lstm_team.h plan_exact(): the sequences run as chains of ≤ 8 rows (one XCD team each) on the exact fp32 VALU
        # recurrence at every B; beyond 64 the chains queue, and the queue holds 32 (raises here, ahead of any launch)
        team_plan(B, True, True)
    # sequence packing (learner/ingest.py): per-(step, row) episode-start flags, time-major (S, B) u8 — the team
    # recurrence zeroes h, c before a flagged step (forward) and stops the gradient there (backward)
    rst = reset_t.reshape(S, B) if reset_t is not None else None
    h0, c0 = h0.contiguous(), c0.contiguous()
    f = _forward(fp, W, P, units_t, env_t, h0, c0, B, S, rst)
    hd = _heads_loss(fp, W, f, act_t, msk_t, adv_t, ret_t, lpo_t, nret_t, norms, B, S, vt_t)
    heads_done = torch.cuda.Event()
    heads_done.record(torch.cuda.current_stream(units_t.device))
    grads = _backward(fp, W, P, f, hd, units_t, env_t, h0, c0, B, S, gout, rst, heads_done)
    return hd.part, hd.logp, grads


class PipelinedPolicyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fp, units, env, actions, masks, adv, ret, logp_old, nret, norms, h0, c0, reset, vt, *params):
        P = dict(zip(fp.param_names, params))
        B, S, U, _ = units.shape
        N = B * S
        tm = (lambda x: x.reshape(B, S, *x.shape[1:]).transpose(0, 1).reshape(N, *x.shape[1:]).contiguous())
        units_t = units.transpose(0, 1).reshape(N, U, 10).contiguous()
        env_t = env.transpose(0, 1).reshape(N, 3).contiguous()
        W = fp.weight_images().refresh(fp.C)
        rst_t = reset.reshape(B, S).transpose(0, 1).reshape(N).contiguous() if reset is not None else None
        part, logp, grads = fused_step_tm(fp, W, P, units_t, env_t, tm(actions), tm(masks), tm(adv), tm(ret),
                                          tm(logp_old), tm(nret), norms, h0, c0, B, S, reset_t=rst_t,
                                          vt_t=tm(vt.reshape(N, 4)) if vt is not None else None)
        ctx.grads = [grads.get(nm) for nm in fp.param_names]
        ctx.fp = fp
        logp_b = logp.view(S, B).t().reshape(N)        # back to batch-major (B·S) row order
        ctx.mark_non_differentiable(logp_b)
        return part.sum(0), logp_b

    @staticmethod
    def backward(ctx, gpart, _glogp):
        ctx.fp.apply_direct_grads(ctx.grads, gpart[15])
        ctx.grads = None
        return (None,) * (14 + len(ctx.fp.param_names))


def train_direct(fp, batch_tm: Dict[str, torch.Tensor], B: int, S: int) -> torch.Tensor:
    """One learner step without autograd: gradients are ADDED into the parameters' ``.grad`` (views of the flat
    gradient buffer), ``fp.grad_mask`` marks which parameters got one. ``batch_tm`` holds time-major rows
    (``units (N,U,10)``, ``env (N,3)``, ``actions``/``masks (N,A)`` u8, ``adv``/``ret``/``logp_old``/``norm_ret``
    (N,)) plus ``h0``/``c0 (B,H)``. Returns the metrics vector (16,) laid out as :data:`METRIC_NAMES`."""
    C = fp.C
    lc = fp.loss_cfg
    N = B * S
    dev = batch_tm['units'].device
    norms = fp.scratch('norms', (8,), torch.float32, dev)
    # the loss normalisers only feed the heads/loss kernel (after the forward recurrence, which runs on the side
    # stream and is waited for by the main stream): computed on that stream, beside the encoder and pre-RNN chain
    main = torch.cuda.current_stream(dev)
    sL = fp.side_stream()
    sL.wait_stream(main)
    with torch.cuda.stream(sL):
        C.loss_prep(batch_tm['actions'], fp.loss_prep_ws(dev), norms)
        if lc.compat_value_bug and lc.vf_coef > 0:
            # the reference's value target is the LAST sequence's returns broadcast over the batch (optimizer.py:603,
            # SURVEY §2.10-2): Σ G_last and Σ G_last² of row b = B-1 for the heads kernel and the loss assembly
            g_last = batch_tm['ret'].view(S, B)[:, B - 1]
            norms[6:8] = torch.stack([g_last.sum(), (g_last * g_last).sum()])
    W = fp.weight_images().refresh(C)
    P = dict(zip(fp.param_names, fp.params))
    H = fp.cfg.hidden
    h0 = batch_tm.get('h0')
    c0 = batch_tm.get('c0')
    if h0 is None:
        h0 = torch.zeros(B, H, device=dev)
        c0 = torch.zeros(B, H, device=dev)
    gout = {nm: P[nm].grad for nm in DIRECT_GEMM_GRADS if nm in P}
    vt = batch_tm.get('vt') if getattr(lc, 'vtrace', False) else None
    if getattr(lc, 'vtrace', False) and vt is None:
        raise ValueError('LossConfig.vtrace needs the per-row vt field (learner/optimizer.py advantages="vtrace-step")')
    part, _, grads = fused_step_tm(fp, W, P, batch_tm['units'], batch_tm['env'], batch_tm['actions'],
                                   batch_tm['masks'], batch_tm['adv'], batch_tm['ret'], batch_tm['logp_old'],
                                   batch_tm['norm_ret'], norms, h0, c0, B, S, gout=gout,
                                   reset_t=batch_tm.get('reset'), vt_t=vt)
    fp.apply_direct_grads([grads.get(nm) for nm in fp.param_names], None,
                          written=set(gout) | set(fp.early_applied))
    out = torch.empty(16, device=dev)
    C.loss_assemble(part, norms, N, 0 if lc.algo == 'ppo' else 1, float(lc.entropy_coef), float(lc.vf_coef), out,
                    S=S, compat_value_bug=bool(lc.compat_value_bug))
    if fp.vtrace_stats is not None:
        st = fp.vtrace_stats.sum(0)
        out[12:15] = st[:3] / st[3].clamp_min(1.0)
    return out


def forward_logp_value(fp, units_t, env_t, act_t, msk_t, h0, c0, B: int, S: int,
                       reset_t: Optional[torch.Tensor] = None):
    """The policy's log-prob of the sampled actions and its value, per time-major row (row = t·B + b), at the weights
    in the flat buffer NOW (in stream order) — :func:`_forward`, the forward part of :func:`fused_step_tm`, then the
    heads kernel; no backward. The learner's ``policy_old`` (reference optimizer.py:279, 474): once per iteration,
    before its minibatches, the iteration's experience is evaluated at the iteration's starting weights
    (learner/optimizer.py ``old_logp='learner'``). Returns (logp (N,) f32, value (N,) f32)."""
    C = fp.C
    N = B * S
    dev = units_t.device
    W = fp.weight_images().refresh(C)
    P = dict(zip(fp.param_names, fp.params))
    rst = reset_t.reshape(S, B) if reset_t is not None else None
    f = _forward(fp, W, P, units_t, env_t, h0.contiguous(), c0.contiguous(), B, S, rst)
    zero = fp.scratch('fwd_zero', (N,), torch.float32, dev)
    norms = fp.scratch('fwd_norms', (8,), torch.float32, dev)
    # the heads kernel's selected-action log-prob (its loss partials / gradients are not used here)
    _, _, _, lp = C.heads_loss(f.z, f.emb, act_t, msk_t, zero, zero, zero, zero, norms, 0, False, S, B, 0.1, 0.0, 0.0,
                               dz_bf16=False, precise=fp.exact)
    return lp, f.z[:, 149].contiguous()
