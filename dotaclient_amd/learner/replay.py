"""On-HBM experience replay: a preallocated device ring buffer of training sequences.

BASELINE.json config 5 asks for a replay buffer sized for the MI355X's 288 GB of HBM3E. The reference has no
replay at all — every iteration trains on exactly the ``seq_per_epoch`` freshly consumed sequences, on the CPU
(optimizer.py:433-483). :class:`HbmReplay` keeps every field the learner step reads as one preallocated tensor
per field on the GPU (``(capacity, seq_len, …)``), so

* ingest is one pinned host→device copy per field per iteration (``add``), written at the ring cursor;
* a minibatch is an on-device ``index_select`` of ``B`` rows (``sample``) — no host round trip, no allocation;
* capacity is chosen from a byte budget (``capacity_for_bytes``): one LSTM-512 1v1 sequence of 1400 steps is
  ≈2.4 MB, so 200 GB holds ≈80k sequences (≈115 M timesteps).

Sampling is uniform over the filled part, optionally restricted to the ``recent`` newest sequences
(``sampler='uniform'``), or — on a ``prioritized`` ring — a mixture (``sampler='mixture'``, ops/replay.py): a share
``recent_frac`` of the draws uniform over the ``recent`` newest sequences, the rest proportional to a per-sequence
priority over the whole ring. The priority ``(eta·max|A| + (1 − eta)·mean|A| + eps)^alpha`` comes from the in-step
V-trace advantages of the step that last trained on the sequence (``update_priorities``); new sequences enter at the
current maximum. ``priority_beta`` > 0 adds the importance-sampling correction of prioritised replay: every draw's
weight ``(size·q)^(−beta) / max`` over the minibatch (ops/replay.py), written by the same sampling pass into a fixed
buffer (``seq_weight``) that the learner step multiplies into the sequence's policy, value and entropy terms;
``priority_beta_anneal`` = N moves beta linearly to 1 over N iterations (``set_iteration``). The priorities themselves
never see the weights. Sampler, priorities and their statistics live on the replay's device: no host sync per step.
Off-policy correction: the PPO ratio against the stored behaviour ``logp_old``, and — with the in-step V-trace
(``vtrace``, learner/optimizer.py advantages='vtrace-step') — every sampled sequence's advantages and value targets
recomputed at the weights being trained, with truncated importance weights against that behaviour log-prob.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..constants import UnitLayout

_F32 = torch.float32


def field_specs(S: int, layout: UnitLayout, hidden: Optional[int], reset: bool = False, vtrace: bool = False):
    U = layout.max_units
    A = 21 + U
    spec = {
        'env': ((S, 3), _F32), 'units': ((S, U, 10), _F32), 'actions': ((S, A), torch.uint8),
        'masks': ((S, A), torch.uint8), 'ret': ((S,), _F32), 'norm_ret': ((S,), _F32), 'adv': ((S,), _F32),
        'logp_old': ((S,), _F32), 'valid': ((S,), _F32),
    }
    if reset:                       # sequence packing: episode-start flags (learner/ingest.py SequencePacker)
        spec['reset'] = ((S,), torch.uint8)
    if vtrace:                      # in-step V-trace rows {reward, bootstrap, valid, last}: replayed sequences get
        spec['vt'] = ((S, 4), _F32)  # their advantages recomputed at every sampling, from the weights being trained
    if hidden:
        spec['h0'] = ((hidden,), _F32)
        spec['c0'] = ((hidden,), _F32)
    return spec


def bytes_per_sequence(S: int, layout: UnitLayout, hidden: Optional[int], reset: bool = False,
                       vtrace: bool = False, prioritized: bool = False) -> int:
    n = 0
    for shape, dt in field_specs(S, layout, hidden, reset, vtrace).values():
        k = 1
        for d in shape:
            k *= d
        n += k * torch.tensor([], dtype=dt).element_size()
    return n + 8 + (4 if prioritized else 0)     # version (+ the fp32 priority of a prioritised ring)


class HbmReplay:
    def __init__(self, capacity: int, S: int, layout: UnitLayout, hidden: Optional[int], device, seed: int = 0,
                 reset: bool = False, vtrace: bool = False, prioritized: bool = False, sampler: str = 'uniform',
                 recent_frac: float = 0.5, priority_alpha: float = 0.6, priority_eta: float = 0.9,
                 priority_eps: float = 1e-3, priority_beta: float = 0.0, priority_beta_anneal: int = 0):
        if capacity < 1:
            raise ValueError('replay capacity must be >= 1')
        if sampler not in ('uniform', 'mixture'):
            raise ValueError(f"sampler must be 'uniform' or 'mixture', got {sampler!r}")
        if sampler == 'mixture' and not prioritized:
            raise ValueError("sampler='mixture' needs prioritized=True (the per-sequence priority vector)")
        if not 0.0 <= recent_frac <= 1.0:
            raise ValueError(f'recent_frac must lie in [0, 1], got {recent_frac}')
        if priority_alpha < 0 or not 0.0 <= priority_eta <= 1.0 or priority_eps <= 0:
            raise ValueError('priority_alpha >= 0, 0 <= priority_eta <= 1 and priority_eps > 0 are required')
        if not 0.0 <= priority_beta <= 1.0 or priority_beta_anneal < 0:
            raise ValueError(f'priority_beta must lie in [0, 1] and priority_beta_anneal be >= 0, got {priority_beta}, '
                             f'{priority_beta_anneal}')
        if priority_beta > 0 and sampler != 'mixture':
            raise ValueError("priority_beta > 0 (importance-sampling weights) needs sampler='mixture': the uniform "
                             "sampler draws without bias and has no weights")
        self.capacity = int(capacity)
        self.S = S
        self.device = torch.device(device)
        self.specs = field_specs(S, layout, hidden, reset, vtrace)
        self.data = {k: torch.zeros((self.capacity,) + shape, dtype=dt, device=self.device)
                     for k, (shape, dt) in self.specs.items()}
        self.version = torch.full((self.capacity,), -1, dtype=torch.long, device=self.device)
        self.cursor = 0
        self.size = 0
        self.inserted = 0
        self._g = torch.Generator(device=self.device).manual_seed(seed)
        # captured learner steps sample this pool through sample_into (host generator, one copy) instead of
        # sample_indices (the device generator); off by default so sample_indices' stream of indices stays the one
        # the learner uses (tests replay it)
        self.host_sampling = False
        self.prioritized = bool(prioritized)
        self.sampler = sampler
        self.recent_frac = float(recent_frac)
        self.priority_alpha, self.priority_eta = float(priority_alpha), float(priority_eta)
        self.priority_eps = float(priority_eps)
        self.current_version = 0        # newest version added: the sampler's age statistic counts from it
        # importance-sampling weights: off at beta = 0 (nothing about sampling or the step changes), else for good —
        # an annealed beta moves, the switch does not, so a captured step stays wired to the weight buffer
        self.priority_beta0, self.priority_beta_anneal = float(priority_beta), int(priority_beta_anneal)
        self.beta = self.priority_beta0
        self.weighted = self.priority_beta0 > 0
        if self.prioritized:
            from ..ops.replay import SamplerState
            # one fp32 priority per slot (0 = unfilled): a separate attribute, not a field the learner step gathers
            self.priority = torch.zeros(self.capacity, dtype=_F32, device=self.device)
            self.priority_nonfinite = torch.zeros(1, dtype=_F32, device=self.device)    # non-finite p_raw so far
            self.sampler_state = SamplerState(self.capacity, self.device, seed)

    @staticmethod
    def capacity_for_bytes(budget: float, S: int, layout: UnitLayout, hidden: Optional[int], reset: bool = False,
                           vtrace: bool = False, prioritized: bool = False) -> int:
        return max(1, int(budget // bytes_per_sequence(S, layout, hidden, reset, vtrace, prioritized)))

    @property
    def nbytes(self) -> int:
        n = sum(t.numel() * t.element_size() for t in self.data.values()) + self.version.numel() * 8
        return n + (self.priority.numel() * 4 if self.prioritized else 0)

    def __len__(self):
        return self.size

    # ------------------------------------------------------------------------------------------------
    def add(self, batch: Dict[str, torch.Tensor], version: int = 0):
        """Append ``n`` sequences (host or device tensors, leading dim n) at the ring cursor (wrapping)."""
        n = int(next(iter(batch.values())).shape[0])
        if n > self.capacity:
            batch = {k: v[-self.capacity:] for k, v in batch.items()}
            n = self.capacity
        first = min(n, self.capacity - self.cursor)
        spans = [(self.cursor, 0, first)]
        if first < n:
            spans.append((0, first, n - first))
        for k, dst in self.data.items():
            src = batch.get(k)
            if src is None and k == 'reset':        # unpacked sequences: no episode starts inside
                for d0, _, cnt in spans:
                    dst[d0:d0 + cnt].zero_()
                continue
            src = batch[k]
            if src.device.type == 'cpu' and self.device.type == 'cuda' and not src.is_pinned():
                src = src.pin_memory()
            for d0, s0, cnt in spans:
                dst[d0:d0 + cnt].copy_(src[s0:s0 + cnt], non_blocking=True)
        for d0, _, cnt in spans:
            self.version[d0:d0 + cnt] = int(version)
            if self.prioritized:
                # new rows enter at the maximum priority the last sampling pass found (1.0 before any): a device
                # scalar broadcast into the slice, no host sync
                self.priority[d0:d0 + cnt] = self.sampler_state.max_priority
        self.current_version = max(self.current_version, int(version))
        self.cursor = (self.cursor + n) % self.capacity
        self.size = min(self.capacity, self.size + n)
        self.inserted += n
        return n

    def prefill(self) -> int:
        """Fill the rest of the ring with copies of the sequences it already holds (device-to-device, doubling
        spans: ≈2 bytes moved per byte filled, so 100 GB takes tens of ms at HBM rate) and mark the copies as
        version -1. Benchmarks use it so a minibatch gathers from the whole ``capacity``-sized pool — the TLB and
        HBM-page spread of a full 100-200 GB replay — from the first timed step, not from a few GB of fresh data.
        New sequences keep landing at the cursor and overwrite the copies oldest-first. Returns the rows written."""
        if self.size == 0:
            raise RuntimeError('prefill needs at least one added sequence')
        if self.size >= self.capacity:
            return 0
        # the held sequences are the ring's first `size` rows (the cursor has not wrapped yet)
        have, wrote = self.size, 0
        while have < self.capacity:
            n = min(have, self.capacity - have)
            for v in self.data.values():
                v[have:have + n].copy_(v[:n])
            self.version[have:have + n] = -1
            if self.prioritized:
                self.priority[have:have + n].copy_(self.priority[:n])
            have += n
            wrote += n
        self.size = self.capacity
        return wrote

    @property
    def fill_fraction(self) -> float:
        return self.size / self.capacity

    def _window(self, recent: Optional[int]):
        m = self.size if not recent else min(self.size, int(recent))
        return m

    def sample_indices(self, B: int, recent: Optional[int] = None) -> torch.Tensor:
        if self.size == 0:
            raise RuntimeError('replay is empty')
        if self.sampler == 'mixture':
            return self._sample_mixture(torch.empty(B, dtype=torch.long, device=self.device), recent)
        m = self._window(recent)
        r = torch.randint(0, m, (B,), device=self.device, generator=self._g)
        # newest-first window ending at the cursor: position (cursor - 1 - r) mod capacity
        return (self.cursor - 1 - r) % self.capacity

    def sample_into(self, out: torch.Tensor, recent: Optional[int] = None) -> torch.Tensor:
        """Sample ``out.numel()`` pool positions (same window as :meth:`sample_indices`) with a host generator and
        write them into the device tensor ``out`` with ONE pinned host→device copy on the current stream — instead
        of the device RNG + two index-arithmetic kernels + a copy (≈26 µs of launches per learner step). The pinned
        slots form a ring; a slot is refilled only after its previous copy has run."""
        if self.size == 0:
            raise RuntimeError('replay is empty')
        if self.sampler == 'mixture':
            return self._sample_mixture(out, recent)
        B = out.numel()
        if out.device.type != 'cuda':
            out.copy_(self.sample_indices(B, recent))
            return out
        ring = self.__dict__.get('_pin_ring')
        if ring is None or ring[0][0].numel() != B:
            ring = self._pin_ring = [[torch.empty(B, dtype=torch.long, pin_memory=True), None] for _ in range(4)]
            self._pin_pos = 0
            self._host_rng = np.random.default_rng(int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
        slot = ring[self._pin_pos]
        self._pin_pos = (self._pin_pos + 1) % len(ring)
        if slot[1] is not None:
            slot[1].synchronize()
        r = self._host_rng.integers(0, self._window(recent), B)
        slot[0].numpy()[:] = (self.cursor - 1 - r) % self.capacity
        out.copy_(slot[0], non_blocking=True)
        ev = slot[1] = slot[1] or torch.cuda.Event()
        ev.record()
        return out

    def set_iteration(self, iteration: int) -> float:
        """The importance-sampling exponent of learner iteration ``iteration`` (0-based): constant, or linear from
        ``priority_beta`` to 1 over ``priority_beta_anneal`` iterations. Returns it."""
        if self.weighted and self.priority_beta_anneal > 0:
            t = min(1.0, max(0.0, iteration / self.priority_beta_anneal))
            self.beta = self.priority_beta0 + (1.0 - self.priority_beta0) * t
        return self.beta

    def seq_weight(self, B: int) -> Optional[torch.Tensor]:
        """The last sampling pass's importance weights of a ``B``-sequence minibatch: a view at a fixed address of the
        sampler state's buffer (what a captured step is wired to); None when the weights are off."""
        if not self.weighted:
            return None
        w = self.sampler_state.is_weight
        if B > w.numel():
            raise ValueError(f'importance-sampling weights: at most {w.numel()} sequences per minibatch (got {B})')
        return w[:B]

    def _sample_mixture(self, out: torch.Tensor, recent: Optional[int] = None, u_out=None) -> torch.Tensor:
        """The mixture sampler (ops/replay.py) into ``out`` (int64 on the replay's device — a captured step's static
        index buffer, or a fresh tensor): on the GPU two launches reading the priorities where they are, the draw
        counter kept on the device; on the CPU the float64 reference fed from this replay's generator. Leaves the
        pass's maximum priority and statistics in ``sampler_state``."""
        from ..ops import replay as R
        st = self.sampler_state
        w_out = self.seq_weight(out.numel())
        if self.device.type == 'cuda':
            return R.sample_mixture(self.priority, self.version, st, out, self.size, self.cursor, recent,
                                    self.recent_frac, self.current_version, u_out,
                                    beta=self.beta if self.weighted else 0.0,
                                    w_out=st.is_weight if self.weighted else None)
        u = torch.rand(out.numel(), 2, generator=self._g)
        if u_out is not None:
            u_out.copy_(u)
        idx, stats = R.sample_mixture_reference(self.priority, self.size, self.cursor, self.capacity, recent,
                                                self.recent_frac, u, self.version, self.current_version)
        st.max_priority.fill_(float(self.priority.max()))
        st.stats[:3].copy_(stats)
        st.stats[3] = float(st.max_priority)
        st.counter += 1
        if w_out is not None:
            w, ws = R.importance_weights_reference(self.priority, idx, self.size, self.cursor, self.capacity, recent,
                                                   self.recent_frac, self.beta)
            w_out.copy_(w)
            st.stats[R.N_STATS:R.N_STATS + R.N_STATS_IS].copy_(ws)
        return out.copy_(idx)

    def update_priorities(self, idx: torch.Tensor, pf: torch.Tensor):
        """Store the priorities ``pf[0]`` of the sequences ``idx`` a step just trained on (``pf`` (2, B) f32: P and the
        non-finite flags, ops/replay.py) — in stream order, no sync, no allocation on the GPU."""
        from ..ops.replay import scatter_priorities
        scatter_priorities(self.priority, idx, pf.to(self.device), self.priority_nonfinite)

    def gather(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {k: v.index_select(0, idx) for k, v in self.data.items()}

    def sample(self, B: int, recent: Optional[int] = None) -> Dict[str, torch.Tensor]:
        return self.gather(self.sample_indices(B, recent))
