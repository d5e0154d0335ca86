"""Learner engine: one optimizer step (forward → loss → backward → DP all-reduce → clip + Adam).

This is the inner hot loop of the reference's ``DotaOptimizer.train`` (optimizer.py:565-688), re-organised around
flat parameter/gradient buffers so that the data-parallel reduction is a few bucketed RCCL collectives and the
optimizer is one fused HIP kernel pair.

Backends for the model math:

* ``'fused'`` (default on GPU): :class:`~dotaclient_amd.models.fused.FusedPolicy` — every product of the step in a
  hand-written gfx950 HIP kernel (entity encoder, attention block, forward / ∂X chains, recurrence, heads + loss,
  split-K weight-gradient GEMMs, clip + Adam); no vendor GEMM.
* ``'torch'``: the eager reference model (``models.policy.Policy``, the oracle): fp32, or under bf16 autocast on GPU
  with ``precision='bf16'`` (the only way a bf16 learner runs: the fused step has no bf16 branch).

``precision``: ``'fp32-exact'`` — the reference's training precision (optimizer.py:281 trains the fp32 module) with
every product an IEEE fp32 FMA; the default of the CLI, the presets and ``bench.py`` (``OptimizerConfig.precision``).
``'fp32'`` (this class's default, kept for the many short-horizon tests) keeps activations, gradients and
accumulation in fp32 with bf16x3-split MFMA operands (``models/fused.py``); ``'bf16'`` = torch backend under autocast.

Batches are dicts of device tensors (see :func:`dotaclient_amd.learner.synthetic.make_batch` for the schema):
``env (B,S,3) f32``, ``units (B,S,U,10) f32``, ``actions``/``masks (B,S,A) u8`` (flat ``enum|x|y|target_unit``),
``adv``/``ret``/``logp_old``/``norm_ret (B,S) f32`` and for recurrent policies ``h0``/``c0 (B,H) f32``.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from ..models.policy import Policy
from ..parallel.dp import DataParallel, FlatParams
from .graphs import StepGraphs
from .losses import ppo_loss, split_heads, vpg_loss
from .optim import FlatAdam


def _gather_rows(data, fields, idx):
    """Sequences ``idx`` of the batch-major ``fields`` of ``data`` as time-major rows, plus their ``h0`` / ``c0``:
    one HIP launch for every field (ops/csrc/glue.hip replay_gather)."""
    from .. import ops
    names = list(fields) + [k for k in ('h0', 'c0') if k in data]
    return dict(zip(names, ops.require().replay_gather([data[k] for k in names], len(fields), idx)))


@dataclass

class LossConfig:
    algo: str = 'ppo'                 # 'ppo' (north star) | 'vpg' (reference objective)
    learning_rate: float = 1e-4       # optimizer.py:778
    entropy_coef: float = 0.01        # optimizer.py:779
    vf_coef: float = 0.5              # optimizer.py:780
    clip_eps: float = 0.1             # e_clip, optimizer.py:239
    gamma: float = 0.98               # optimizer.py:382
    gae_lambda: float = 0.95
    max_grad_norm: float = 0.5        # optimizer.py:215
    compat_value_bug: bool = False    # optimizer.py:603 broadcast quirk
    # PPO policy term: 'clip' = the clipped surrogate against logp_old (fresh experience: logp_old is the learner's own
    # log-prob at the iteration's weights, learner/optimizer.py old_logp='learner'); 'tis' = off-policy policy
    # gradient with the truncated importance weight min(1, π/π_old) (replayed experience, V-trace style)
    offpolicy: str = 'clip'
    # V-trace inside the step: the advantages and value targets of every minibatch recomputed from the step's own
    # values and log-probs against the actor's behaviour log-prob (``logp_old``) — batches carry the per-row ``vt``
    # field {reward, bootstrap, valid, last} (learner/optimizer.py advantages='vtrace-step'); ``adv`` / ``ret`` unused
    vtrace: bool = False
    vtrace_rho_bar: float = 1.0
    vtrace_c_bar: float = 1.0


class Learner:
    def __init__(self, policy: Policy, loss_cfg: LossConfig, device='cpu', backend: str = 'auto',
                 bucket_cap_mb: float = 8.0, overlap: bool = True, dp: bool = True, precision: str = 'fp32'):
        if precision not in ('fp32', 'bf16', 'fp32-exact'):
            raise ValueError(f'precision must be fp32, fp32-exact or bf16, got {precision!r}')
        self.device = torch.device(device)
        self.cfg = loss_cfg
        self.precision = precision
        self.policy = policy.to(self.device)
        auto = backend == 'auto'
        if auto:
            backend = 'fused' if self.device.type == 'cuda' else 'torch'
        self.backend = backend
        self.flat = FlatParams(self.policy, device=self.device)
        self.dp = DataParallel(self.policy, flat=self.flat, bucket_cap_mb=bucket_cap_mb, overlap=overlap,
                               broadcast=dp)
        self.opt = FlatAdam(self.flat, lr=loss_cfg.learning_rate, max_grad_norm=loss_cfg.max_grad_norm,
                            use_kernels=self.device.type == 'cuda')
        self.model = self.policy
        if backend == 'fused':
            from ..models.fused import FusedPolicy
            fused = FusedPolicy(self.policy, loss_cfg, precision=precision)
            if fused.use_pipeline():
                self.model = fused
                self.model.attach_flat(self.flat.flat)
            elif auto:
                self.backend = backend = 'torch'     # a configuration the kernels do not cover
            else:
                raise ValueError(f'backend fused: no kernel path for {self.policy.config} at {precision}')
        self.counts = self.policy.layout.action_counts()
        self.n_steps = 0
        self.graphs = StepGraphs(self.device)     # captured steps (see enable_graph)
        self._graph_warmup = 0
        self._split: Optional[bool] = None        # two-phase DP step; decided on first use (_split_mode)
        self._err_any: Optional[torch.Tensor] = None    # sticky DP-wide error flag, made by the first DP sync

    def enable_graph(self, warmup: int = 2):
        """Capture forward + loss + backward of the direct fused step in a hipGraph after ``warmup`` eager steps.
        The step is a few dozen hand-written kernels (no vendor GEMM) on several streams; a replay spares the
        Python and launch cost of each of them. The DP all-reduce and the fused Adam stay outside the graph (RCCL
        collectives are not captured). Inputs are copied into the static buffers of their key (learner/graphs.py)
        before each replay."""
        if not self.direct():       # only the autograd-free step is captured: it has no work in a backward thread
            return False
        self._graph_warmup = max(1, int(warmup))
        return True

    @property
    def graph(self):
        """The most recently captured step graph (None before any capture and once its step was released)."""
        return self.graphs.last

    # ------------------------------------------------------------------------------------------------
    def _autocast(self):
        if self.backend == 'torch' and self.device.type == 'cuda' and self.precision == 'bf16':
            return torch.autocast('cuda', dtype=torch.bfloat16)
        return contextlib.nullcontext()

    def hidden_from_batch(self, batch):
        if not self.policy.is_recurrent:
            return None
        return (batch['h0'].unsqueeze(0).contiguous(), batch['c0'].unsqueeze(0).contiguous())

    def loss(self, batch: Dict[str, torch.Tensor]):
        cfg = self.cfg
        stable = not self.policy.config.compat_bugs
        if self.backend == 'fused':
            return self.model.loss(batch, cfg)
        with self._autocast():
            logits, values, _ = self.model.forward_packed(batch['env'], batch['units'], self.hidden_from_batch(batch),
                                                          reset=batch.get('reset'))
        logits = {k: v.float() for k, v in logits.items()}
        values = values.float()
        actions = split_heads(batch['actions'], self.counts)
        masks = split_heads(batch['masks'], self.counts)
        if cfg.algo == 'ppo':
            adv, ret, extra = batch['adv'], batch['ret'], {}
            if cfg.vtrace:
                adv, ret, extra = self._vtrace_torch(batch, logits, values, masks, actions)
            loss, metrics = ppo_loss(logits, values, actions, masks, adv, ret, batch['logp_old'],
                                     cfg.clip_eps, cfg.entropy_coef, cfg.vf_coef, stable=stable,
                                     offpolicy=cfg.offpolicy, seq_weight=getattr(self, '_seq_weight', None))
            metrics.update(extra)
            return loss, metrics
        if getattr(self, '_seq_weight', None) is not None:
            raise ValueError('per-sequence loss weights (replay priority_beta > 0) are not defined for the VPG loss')
        return vpg_loss(logits, values, actions, masks, batch['norm_ret'], batch['ret'], cfg.entropy_coef,
                        cfg.vf_coef, compat_value_bug=cfg.compat_value_bug, stable=stable)

    def _vtrace_torch(self, batch, logits, values, masks, actions):
        """The torch oracle of the fused step's in-step V-trace (ops/scan.py vtrace_step over time-major rows): the
        step's own (detached) values and log-probs of the recorded actions against ``logp_old``; advantages
        normalised over the valid rows. Returns (adv (B,S), ret (B,S), off-policy metrics)."""
        from ..constants import EPS
        from ..ops.scan import vtrace_step
        from .losses import sampled_logp
        cfg = self.cfg
        B, S = batch['env'].shape[:2]
        tm = (lambda x: x.detach().float().reshape(B, S, *x.shape[2:]).transpose(0, 1).reshape(B * S, *x.shape[2:]))
        with torch.no_grad():
            lp = sampled_logp(logits, actions, masks, stable=not self.policy.config.compat_bugs)
            adv, ret, st = vtrace_step(tm(values.squeeze(-1)).cpu(), tm(lp).cpu(), tm(batch['logp_old']).cpu(),
                                       tm(batch['vt']).cpu(), B, S, cfg.gamma, cfg.gae_lambda, cfg.vtrace_rho_bar,
                                       cfg.vtrace_c_bar)
            dev = batch['env'].device
            pc = getattr(self, '_priority_cfg', None)
            if pc is not None:      # the step trains from a prioritised replay (_step_prioritized)
                from ..ops.replay import priority_from_advantages
                self._seq_priority = torch.stack(priority_from_advantages(adv, tm(batch['vt'])[:, 2].cpu(), B, S,
                                                                          *pc)).to(dev)
            back = (lambda x: x.reshape(S, B).t().contiguous().to(dev))
            adv, ret = back(adv), back(ret)
            v = batch['vt'][..., 2].float()
            n = v.sum().clamp_min(1.0)
            mu = (adv * v).sum() / n
            sd = (((adv - mu) ** 2 * v).sum() / n).sqrt()
            adv = ((adv - mu) / (sd + EPS)) * v
            s = st.sum(0)
            extra = {'offpolicy/rho_mean': (s[0] / s[3].clamp_min(1)).to(dev),
                     'offpolicy/rho_truncated': (s[1] / s[3].clamp_min(1)).to(dev),
                     'offpolicy/behaviour_kl': (s[2] / s[3].clamp_min(1)).to(dev)}
        return adv, ret, extra

    def _fwd_bwd(self, batch):
        self.dp.zero_grad()
        loss, metrics = self.loss(batch)
        loss.backward()
        if self.backend == 'fused' and getattr(self.model, 'direct_used', False):
            # the fused Functions accumulate straight into the flat gradient buffer (no per-parameter autograd
            # hooks fire); tell the DP layer which parameters received a gradient
            self.dp.has_grad.copy_(self.model.grad_mask)
        return {k: v.detach() for k, v in metrics.items()}

    # ---- direct (autograd-free) fused LSTM step ------------------------------------------------------
    def direct(self) -> bool:
        """The fused LSTM policy runs the autograd-free step (models/pipelined.py:train_direct)."""
        return self.backend == 'fused' and self.device.type == 'cuda' and self.model.use_pipeline()

    STEP_FIELDS = ('units', 'env', 'actions', 'masks', 'adv', 'ret', 'logp_old', 'norm_ret')

    @staticmethod
    def batch_to_time_major(batch):
        """Batch-major ``(B,S,…)`` fields → time-major rows ``(S·B,…)`` (row = t·B + b)."""
        B, S = batch['env'].shape[:2]
        out = {}
        for k in Learner.STEP_FIELDS:
            v = batch.get(k)
            if v is None:
                v = torch.zeros(B, S, device=batch['env'].device)
            out[k] = v.transpose(0, 1).reshape(S * B, *v.shape[2:]).contiguous()
        if 'reset' in batch:                # sequence packing: episode-start flags (B,S) u8 → time-major rows
            out['reset'] = batch['reset'].transpose(0, 1).reshape(S * B).contiguous()
        if 'vt' in batch:                   # in-step V-trace rows {reward, bootstrap, valid, last} (B,S,4)
            out['vt'] = batch['vt'].transpose(0, 1).reshape(S * B, 4).contiguous()
        for k in ('h0', 'c0'):
            if k in batch:
                out[k] = batch[k].contiguous()
        return out, B, S

    def gather_time_major(self, replay, idx, S: int):
        """Minibatch of replay rows ``idx`` gathered straight into time-major rows: one index_select per field
        over the pool viewed as (capacity·S, …) — no batch-major copy, no transpose."""
        B = idx.numel()
        fields = self.STEP_FIELDS + tuple(k for k in ('reset', 'vt') if k in replay.data)
        if idx.is_cuda:
            return _gather_rows(replay.data, fields, idx.contiguous())
        rows = (idx.view(1, B) * S + torch.arange(S, device=idx.device, dtype=torch.long).view(S, 1)).reshape(-1)
        out = {}
        for k in fields:
            pool = replay.data[k]
            out[k] = pool.view(-1, *pool.shape[2:]).index_select(0, rows)
        for k in ('h0', 'c0'):
            if k in replay.data:
                out[k] = replay.data[k].index_select(0, idx)
        return out

    def _split_mode(self) -> bool:
        """Data-parallel direct step in two phases: the recurrence / pre-RNN / heads gradients are all-reduced on
        the comm stream while the encoder backward still runs (RCCL over xGMI overlapped with backward). The split
        needs a contiguous early-parameter range (DataParallel.split_buckets).
        ``DCA_DP_SPLIT=1`` forces it without a process group (single-GPU tests of the two-graph mechanics)."""
        if self._split is None:
            force = os.environ.get('DCA_DP_SPLIT') == '1'
            ok = self.direct() and (self.dp.enabled or force) and os.environ.get('DCA_DP_SPLIT', '') != '0'
            if ok:
                early = self.model.early_param_names()
                idx = [i for i, n in enumerate(self.model.param_names) if n in early]
                ok = self.dp.split_buckets(idx) if self.dp.enabled else bool(idx)
            self._split = bool(ok)
        return self._split

    def _direct_body(self, batch_tm, B, S, hook=None):
        self.flat.grad.zero_()
        if hook is None and self._split_mode():
            hook = self.dp.launch_early                   # eager step: launch the early buckets right away
        self.model.split_hook = hook
        try:
            vec = self.model.train_direct(batch_tm, B, S, self.cfg)
        finally:
            self.model.split_hook = None
        self.dp.has_grad.copy_(self.model.grad_mask)
        return vec

    def _metrics_from_vec(self, vec):
        from ..models.pipelined import METRIC_NAMES
        names = [n for n in METRIC_NAMES if (self.cfg.algo == 'ppo' or n not in ('approx_kl', 'clipfrac'))
                 and (self.cfg.vtrace or not n.startswith('offpolicy/'))]
        return {n: vec[METRIC_NAMES.index(n)] for n in names}

    def _graph_ready(self) -> bool:
        return bool(self._graph_warmup) and self.n_steps >= self._graph_warmup

    def _captured(self, key, make_static, fill, rows):
        """The captured direct step of ``key`` (learner/graphs.py): ``make_static()`` makes a new key's static inputs,
        ``fill(static)`` writes this step's into a known key's, ``rows(static)`` → (time-major rows, B, S). The one
        place that decides between the single graph and the split pair around ``dp.launch_early``."""
        split = self._split_mode()
        return self.graphs.step(key, make_static, fill,
                                lambda static, hook: self._direct_body(*rows(static), hook=hook if split else None),
                                between=self.dp.launch_early if split else None)

    def _step_direct_batch(self, batch):
        if not self._graph_ready():
            return self._direct_body(*self.batch_to_time_major(batch))
        B, S = batch['env'].shape[:2]

        def fill(static):
            for k, v in batch.items():
                static[k].copy_(v, non_blocking=True)
        return self._captured(('batch', B, S, tuple(sorted(batch))), lambda: {k: v.clone() for k, v in batch.items()},
                              fill, self.batch_to_time_major)

    def release_graphs(self, replay) -> int:
        """Drop every captured step bound to ``replay`` — call before its storage is reallocated or freed. Returns
        the number of steps released."""
        return self.graphs.release(replay)

    def train_step_replay(self, replay, B: int, recent: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """One DP optimizer step on a minibatch sampled from an on-device replay (``learner.replay.HbmReplay``).
        On the direct fused path the gather itself is part of the captured graph: the sampled positions go straight
        into the graph's own index buffer (one copy)."""
        if getattr(replay, 'prioritized', False):
            return self._step_prioritized(replay, B, recent)
        if self.direct() and self._graph_ready() and getattr(replay, 'host_sampling', False):
            return self._step_replay_key(replay, B, lambda: replay.sample_indices(B, recent),
                                         lambda static: replay.sample_into(static, recent))
        return self.train_step_indices(replay, replay.sample_indices(B, recent))

    def _step_prioritized(self, replay, B: int, recent: Optional[int]) -> Dict[str, torch.Tensor]:
        """A step from a prioritised replay: the replay's sampler fills the index buffer (the captured step's static
        one: the mixture sampler is a kernel writing straight into it, ``host_sampling`` does not apply), the step
        computes the sampled sequences' new priorities from its un-normalised V-trace advantages (fused: the
        ``seq_priority`` kernel inside the step, next to the V-trace kernel; torch: ops/replay.py
        ``priority_from_advantages``) and a scatter stores them behind the step, in stream order. The sampler's
        statistics of this step ride in the returned metrics. Eager and captured steps draw the same index stream.
        With importance-sampling weights (``replay.weighted``) the same sampling pass writes the draws' weights into
        the sampler state's fixed buffer; the step reads its first ``B`` entries (``seq_weight``) in the loss. A
        captured step with weights has a key of its own: its loss kernel is wired to that buffer."""
        update = self.cfg.vtrace and self.cfg.algo == 'ppo'
        sw = replay.seq_weight(B) if getattr(replay, 'weighted', False) else None
        if sw is not None and self.cfg.algo != 'ppo':
            raise ValueError('importance-sampling weights (replay priority_beta > 0) weight the PPO objectives; the '
                             'VPG loss has no weighted form')
        if not update and replay.priority_alpha > 0:
            raise ValueError("a prioritised replay with priority_alpha > 0 needs the in-step V-trace advantages: "
                             "LossConfig(algo='ppo', vtrace=True) (learner/optimizer.py advantages='vtrace-step')")
        fused = self.backend == 'fused'
        # (alpha = 0 without the in-step V-trace: every priority stays at its entry value 1 = (·)^0, nothing to store)
        pc = (replay.priority_eta, replay.priority_alpha, replay.priority_eps) if update else None
        self._priority_cfg = pc
        self._seq_weight = sw
        if fused:
            self.model.priority_cfg = pc
            self.model.seq_weight = sw
        try:
            if self.direct() and self._graph_ready():
                if replay.sampler == 'mixture' or getattr(replay, 'host_sampling', False):
                    fill = (lambda static: replay.sample_into(static, recent))
                else:
                    fill = (lambda static: static.copy_(replay.sample_indices(B, recent)))
                m = self._step_replay_key(replay, B, lambda: replay.sample_indices(B, recent), fill,
                                          weighted=sw is not None)
                idx = self.graphs.static(self._replay_key(replay, B, replay.S, sw is not None))
            else:
                idx = replay.sample_indices(B, recent)
                if self.direct():
                    m = self._finish(self._direct_body(self.gather_time_major(replay, idx, replay.S), B, replay.S))
                else:
                    m = self.train_step(replay.gather(idx))
        finally:
            self._priority_cfg = None
            self._seq_weight = None
            if fused:
                self.model.priority_cfg = None
                self.model.seq_weight = None
        if update:
            # fused: the buffer the step's seq_priority kernel wrote (models/pipelined.py _heads_loss) — the very
            # tensor a captured step is wired to, looked up, never re-made
            replay.update_priorities(idx, self.model._scratch[f'seq_priority_{B}'] if fused else self._seq_priority)
        st = replay.sampler_state.stats.clone()     # one copy: the values below are views of it
        m['replay/recent_draws'], m['replay/age_sum'], m['replay/priority_sum'] = st[0], st[1], st[2]
        m['replay/priority_max'] = st[3]
        if sw is not None:
            m['replay/is_weight_sum'], m['replay/is_weight_min'], m['replay/zero_prob_draws'] = st[4], st[5], st[6]
        return m

    def train_step_indices(self, replay, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One DP optimizer step on the pool sequences ``idx`` (device int64) of ``replay`` — any object with
        ``data`` (field → (capacity, S, …) device tensors at fixed addresses), ``S`` and ``gather(idx)``: the HBM
        replay, or the optimizer's per-iteration pool (epoch permutations over the iteration's sequences)."""
        if not self.direct():
            return self.train_step(replay.gather(idx))
        if self._graph_ready():
            return self._step_replay_key(replay, idx.numel(), lambda: idx, lambda static: static.copy_(idx))
        return self._finish(self._direct_body(self.gather_time_major(replay, idx, replay.S), idx.numel(), replay.S))

    def _replay_key(self, replay, B: int, S: int, weighted: bool = False):
        """Graph-cache key of a step on ``replay``; a step whose loss reads per-sequence weights never shares one
        with a step that does not."""
        key = self.graphs.replay_key(replay, B, S)
        return key + ('is_weight',) if weighted else key

    def _step_replay_key(self, replay, B: int, indices, fill, weighted: bool = False) -> Dict[str, torch.Tensor]:
        """Captured step on ``B`` sequences of ``replay``: the key's static input is its index buffer, a copy of
        ``indices()`` when the key is new and written by ``fill`` from then on."""
        S = replay.S
        return self._finish(self._captured(self._replay_key(replay, B, S, weighted), lambda: indices().clone(), fill,
                                           lambda sidx: (self.gather_time_major(replay, sidx, S), B, S)))

    def _sync_and_step(self):
        """DP reduction + optimizer step. With the fused Adam on a multi-rank job the has-grad average is taken
        inside the optimizer kernels (no separate pass over the gradient buffer after the all-reduce). The fused
        model's persistent-kernel error flag rides in the count-carrying bucket: if the recurrence failed on ANY
        rank, every rank's Adam skips this step on the device (FusedPolicy.check_error raises at the iteration
        boundary) — the reference raises before optimizer.step() (optimizer.py:674-676)."""
        if self.backend == 'fused':
            self.dp.err_flag.copy_(self.model.err)
        fold = self.dp.enabled and self.opt.use_kernels
        self.dp.sync(scale=not fold)
        if self.backend == 'fused' and self.dp.enabled:
            # the reduced flag is non-zero on EVERY rank when any rank's recurrence failed: keep it sticky so that
            # all ranks raise together at the iteration boundary (check_error), not only the failing one
            sticky = self._err_any
            if sticky is None:
                sticky = self._err_any = torch.zeros_like(self.dp.err_flag)
            torch.maximum(sticky, self.dp.err_flag, out=sticky)
        return self.opt.step(self.dp.counts, divide=fold, skip=self.dp.err_flag)

    def check_error(self):
        """Raise (on every DP rank alike) if a persistent kernel failed on any rank since the last call; host sync,
        call at iteration boundaries."""
        self.opt.check_nonfinite()
        if self.backend != 'fused':
            return
        sticky = self._err_any
        if sticky is not None and float(sticky.item()) != 0.0:
            own = int(self.model.err.item())
            sticky.zero_()
            raise RuntimeError(f'persistent kernel error on a data-parallel rank (own code {own}): the step was '
                               'skipped by every rank\'s Adam')
        self.model.check_error()

    def error_flags(self) -> List[torch.Tensor]:
        """The device flags :meth:`check_error` reads (non-finite step, sticky DP error, recurrence error), for a
        caller that snapshots them asynchronously with its other per-iteration values: when the snapshot shows one
        non-zero it calls :meth:`check_error`, whose host syncs then only happen on the failure path."""
        flags = [self.opt.nonfinite]
        if self.backend == 'fused':
            sticky = self._err_any
            if sticky is not None:
                flags.append(sticky)
            flags.append(self.model.err)
        return flags

    def team_stat_tensors(self) -> List[torch.Tensor]:
        """The recurrence's device statistics blocks (ops/lstm.py; empty on the torch backend), for a caller that
        snapshots them asynchronously with its other per-iteration values."""
        if self.backend != 'fused' or self.device.type != 'cuda':
            return []
        return self.model.team_stat_tensors()

    def _finish(self, vec):
        metrics = self._metrics_from_vec(vec.clone())
        # a copy: the optimizer's norm is ONE persistent tensor rewritten by every step, and with deferred metrics the
        # iteration's list is read only after the next iteration's steps were queued
        metrics['grad_norm'] = self._sync_and_step().clone()
        self.n_steps += 1
        return metrics

    def train_step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """One synchronous DP optimizer step. Returns device-resident metric tensors (no host sync)."""
        if self.direct():
            return self._finish(self._step_direct_batch(batch))
        metrics = self._fwd_bwd(batch)
        metrics['grad_norm'] = self._sync_and_step().clone()
        self.n_steps += 1
        return metrics

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate_sequences(self, data: Dict[str, torch.Tensor], n: int, chunk: int = 32):
        """Log-prob of the sampled actions and value of every step of sequences ``0..n-1`` of ``data`` (batch-major
        ``(≥n, S, …)`` fields ``units``, ``env``, ``actions``, ``masks`` (+ ``h0``/``c0``, ``reset``)) at the
        CURRENT weights, in stream order: the learner-side ``policy_old`` of the reference (optimizer.py:279, 474) —
        the PPO ratio's denominator and the GAE / V-trace values of the iteration's experience. Returns (logp (n, S),
        value (n, S)) f32 on the learner's device. The fused path runs the step's forward kernels (fp32-exact: IEEE
        fp32, ``chunk`` ≤ 32 sequences per launch — the exact recurrence's 4 rows per XCD chain); the torch path the
        eager module."""
        S = data['units'].shape[1]
        if self.direct():
            fields = ('units', 'env', 'actions', 'masks') + (('reset',) if 'reset' in data else ())
            lps, vals = [], []
            for i0 in range(0, n, chunk):
                i1 = min(n, i0 + chunk)
                bt = _gather_rows(data, fields, torch.arange(i0, i1, device=self.device, dtype=torch.int64))
                lp, v = self.model.forward_logp_value(bt, i1 - i0, S)
                lps.append(lp.view(S, i1 - i0).t())
                vals.append(v.view(S, i1 - i0).t())
            return torch.cat(lps, 0).contiguous(), torch.cat(vals, 0).contiguous()
        from .losses import sampled_logp
        hidden = None
        if self.policy.is_recurrent and 'h0' in data:
            hidden = (data['h0'][:n].unsqueeze(0).contiguous(), data['c0'][:n].unsqueeze(0).contiguous())
        with self._autocast():
            logits, values, _ = self.model.forward_packed(data['env'][:n], data['units'][:n], hidden,
                                                          reset=data['reset'][:n] if 'reset' in data else None)
        logits = {k: v.float() for k, v in logits.items()}
        lp = sampled_logp(logits, split_heads(data['actions'][:n], self.counts), split_heads(data['masks'][:n],
                                                                                             self.counts),
                          stable=not self.policy.config.compat_bugs)
        return lp.float(), values.float().reshape(n, S)

    def state_dict(self):
        return {'optimizer': self.opt.state_dict(), 'n_steps': self.n_steps}

    def broadcast_state(self, src: int = 0):
        """Make every rank's optimizer state (Adam moments, per-parameter step counts) equal to rank ``src``'s."""
        import torch.distributed as dist
        for t in (self.opt.exp_avg, self.opt.exp_avg_sq, self.opt.steps):
            dist.broadcast(t, src)
        n = torch.tensor([self.n_steps], dtype=torch.int64, device=self.opt.steps.device)
        dist.broadcast(n, src)
        self.n_steps = int(n.item())

    def load_state_dict(self, d):
        self.opt.load_state_dict(d['optimizer'])
        self.n_steps = d.get('n_steps', 0)

    def after_load_weights(self):
        """Call after ``policy.load_state_dict`` so the flat buffers see the new weights."""
        self.flat.rebind()
        if self.backend == 'fused':
            self.model.refresh()
