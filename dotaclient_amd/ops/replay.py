"""Prioritised mixture sampling over the on-HBM replay ring (``csrc/replay_sample.hip``) plus its CPU references.

Every replayed sequence carries a priority ``P = (p_raw + eps)^alpha`` with ``p_raw = eta·max_t|A_t| + (1 − eta)·
mean_t|A_t|`` over its valid rows, ``A`` the UN-normalised in-step V-trace advantages of the step that last trained on
it (ops/scan.py ``vtrace_step``). A sequence without a valid row has ``p_raw = 0``; a non-finite ``p_raw`` is stored as
``eps^alpha`` and flagged. Unfilled ring slots have priority 0.

Each of the ``B`` draws of a minibatch consumes two uniforms ``(u0, u1)`` in ``[0, 1)`` of 24 random bits each:

* ``u0 < recent_frac`` — newest-window draw: uniform over the newest ``m = min(size, recent or size)`` sequences,
  ``r = min(m − 1, floor(u1·m))``, ``idx = (cursor − 1 − r) mod capacity`` (the window of ``HbmReplay.sample_indices``);
* otherwise — prioritised draw over all slots: with ``T = Σ P_i``, ``idx`` is the smallest ``i`` whose inclusive prefix
  sum exceeds ``u1·T``; if rounding leaves none, the last slot with ``P_i > 0``. (``T = 0``, nothing to prioritise:
  the newest-window draw.)

Sums are accumulated in double, in a fixed order, so equal (state, seed, counter) give equal indices. On the GPU the
uniforms come from a counter-based hash (the idiom of ``csrc/actor.hip``): the kernel reads the draw counter from device
memory and writes the next value itself, so a launch changes no host value.

Importance-sampling weights (``beta`` > 0): a slot's probability under the whole mixture, whichever branch drew it, is
``q(i) = f·[i in the newest window]/m + (1 − f)·P_i/T`` (``f = recent_frac``; ``T ≤ 0``: ``[in window]/m``), its weight
``w_i = (size·q(i))^(−beta)``, and a minibatch's weights are divided by their maximum, so they lie in (0, 1] and only
ever scale a sequence's loss down. ``q = 0`` is reachable only through the clamped fall-back paths: such a draw takes
``w = 1`` before the division and is counted. The sampler kernel writes them next to the indices; the CPU form is
:func:`importance_weights_reference`.

On a GPU tensor the HIP kernels run (and the extension is required); on CPU the references below run — they are also
the oracles of the GPU tests.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

BLOCK = 4096            # slots per block sum (csrc/replay_sample.hip kBlock)
MAX_CAPACITY = 1 << 20  # 256 block sums scanned in LDS
N_STATS = 4             # newest-window draws, Σ (current version − version[idx]), Σ P[idx], max priority
N_STATS_IS = 3          # behind them, of the importance weights: Σ w, min w, draws with q = 0
MAX_IS_BATCH = 256      # the largest minibatch of the exact learner: entries of SamplerState.is_weight


def priority_from_advantages(adv: torch.Tensor, valid: torch.Tensor, B: int, S: int, eta: float = 0.9,
                             alpha: float = 0.6, eps: float = 1e-3) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-sequence priorities from TIME-MAJOR rows (r = t·B + b): ``adv`` (B·S,) un-normalised advantages, ``valid``
    (B·S,) > 0 on real rows. float64 arithmetic; returns (P (B,) f32, nonfinite (B,) f32 flags). The oracle of the
    ``seq_priority`` kernel and the torch learner's own path."""
    a = adv.detach().reshape(S, B).double().abs().cpu()
    v = (valid.detach().reshape(S, B) > 0).cpu()
    n = v.sum(0).double()
    amax = torch.where(v, a, torch.zeros_like(a))
    amax = torch.where(torch.isnan(amax), torch.full_like(amax, float('inf')), amax).max(0).values
    mean = torch.where(v, a, torch.zeros_like(a)).sum(0) / n.clamp_min(1.0)
    p_raw = torch.where(n > 0, eta * amax + (1.0 - eta) * mean, torch.zeros_like(mean))
    bad = ~torch.isfinite(p_raw)
    p = torch.where(bad, torch.zeros_like(p_raw), p_raw)
    P = (p + eps) ** alpha
    P = torch.where(bad, torch.full_like(P, float(eps) ** float(alpha)), P)
    return P.float().to(adv.device), bad.float().to(adv.device)


def sample_mixture_reference(priority, size: int, cursor: int, capacity: int, recent: Optional[int],
                             recent_frac: float, u, version=None, current_version: int = 0):
    """The mixture sampler in float64 numpy, the uniforms ``u`` (B, 2) given. Returns (idx (B,) int64 tensor,
    stats (3,) float64 tensor = newest-window draws, Σ (current_version − version[idx]), Σ P[idx])."""
    p = np.asarray(torch.as_tensor(priority).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    u = np.asarray(torch.as_tensor(u).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 2)
    assert p.shape[0] == capacity and 1 <= size <= capacity
    m = size if not recent else min(size, int(recent))
    cum = np.cumsum(p)
    T = cum[-1]
    pos = np.nonzero(p > 0)[0]
    newest = (u[:, 0] < np.float32(recent_frac)) | (T <= 0)
    r = np.minimum(m - 1, np.floor(u[:, 1].astype(np.float64) * m).astype(np.int64))
    idx_new = (cursor - 1 - r) % capacity
    idx_pri = np.searchsorted(cum, u[:, 1].astype(np.float64) * T, side='right')
    if pos.size:
        idx_pri = np.where(idx_pri >= capacity, pos[-1], idx_pri)
    idx = np.where(newest, idx_new, np.minimum(idx_pri, capacity - 1)).astype(np.int64)
    age = 0.0
    if version is not None:
        ver = torch.as_tensor(version).detach().cpu().numpy().astype(np.int64)
        age = float((current_version - ver[idx]).sum())
    stats = np.array([float(newest.sum()), age, float(p[idx].sum())], dtype=np.float64)
    return torch.from_numpy(idx), torch.from_numpy(stats)


def importance_weights_reference(priority, idx, size: int, cursor: int, capacity: int, recent: Optional[int],
                                 recent_frac: float, beta: float):
    """Importance-sampling weights of the drawn slots ``idx`` (B,) in float64 numpy: the oracle of the sampler
    kernel's ``w_out`` and the CPU replay's own path. Returns (w (B,) float64 tensor, normalised by the batch maximum;
    stats (3,) float64 tensor = Σ w, min w — both over the weights rounded to float32, as stored — and the draws with
    q = 0)."""
    p = np.asarray(torch.as_tensor(priority).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    i = np.asarray(torch.as_tensor(idx).detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    assert p.shape[0] == capacity and 1 <= size <= capacity and beta >= 0
    m = size if not recent else min(size, int(recent))
    f = np.float64(np.float32(recent_frac))
    T = np.cumsum(p)[-1]
    win = np.where(((cursor - 1 - i) % capacity) < m, 1.0 / np.float64(m), 0.0)
    q = f * win + (1.0 - f) * (p[i] / T) if T > 0 else win
    zero = ~(q > 0)
    w = np.where(zero, 1.0, np.power(np.float64(size) * np.where(zero, 1.0, q), -np.float64(beta)))
    w = w / w.max()
    w32 = w.astype(np.float32).astype(np.float64)
    stats = np.array([w32.sum(), w32.min(), float(zero.sum())], dtype=np.float64)
    return torch.from_numpy(w), torch.from_numpy(stats)


class SamplerState:
    """Device state of one replay's sampler: the draw counter, the block-sum scratch, the maximum priority and the
    statistics of the last sampling pass, and the importance weights of its draws (``is_weight``: a fixed buffer a
    captured step reads its first ``B`` entries of). Allocated once; a sampling pass allocates nothing."""

    def __init__(self, capacity: int, device, seed: int = 0):
        if capacity > MAX_CAPACITY:
            raise ValueError(f'prioritised replay: at most {MAX_CAPACITY} sequences (got {capacity})')
        dev = torch.device(device)
        nblk = (int(capacity) + BLOCK - 1) // BLOCK
        self.seed = int(seed) & (2 ** 63 - 1)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.block_sum = torch.zeros(nblk, dtype=torch.float64, device=dev)
        self.block_max = torch.zeros(nblk, dtype=torch.float32, device=dev)
        self.max_priority = torch.ones(1, dtype=torch.float32, device=dev)      # 1.0 before any sampling pass
        self.stats = torch.zeros(N_STATS + N_STATS_IS, dtype=torch.float64, device=dev)
        self.is_weight = torch.ones(MAX_IS_BATCH, dtype=torch.float32, device=dev)


def sample_mixture(priority: torch.Tensor, version: torch.Tensor, state: SamplerState, out: torch.Tensor, size: int,
                   cursor: int, recent: Optional[int], recent_frac: float, current_version: int = 0,
                   u_out: Optional[torch.Tensor] = None, beta: float = 0.0,
                   w_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Draw ``out.numel()`` ring positions into ``out`` (int64, the caller's buffer) on the GPU: two launches
    (``csrc/replay_sample.hip``), no host sync, no allocation. Updates ``state`` (counter, max_priority, stats);
    ``u_out`` (B, 2) f32 optionally receives the uniforms used. With ``w_out`` (≥ B f32, e.g. ``state.is_weight``) the
    same pass writes the draws' importance-sampling weights at ``beta`` into its first B entries and their statistics
    into ``state.stats[4:7]``; ``beta`` is a launch argument and may change from pass to pass."""
    from . import require
    m = int(size) if not recent else min(int(size), int(recent))
    if w_out is None and beta:
        raise ValueError('sample_mixture: beta > 0 needs w_out, the buffer the weights go to')
    require().replay_sample(priority, version, state.block_sum, state.block_max, state.counter, state.seed, out,
                            state.max_priority, state.stats, u_out, int(size), int(cursor), m, float(recent_frac),
                            int(current_version), float(beta), w_out)
    return out


def seq_priority(adv: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, S: int, eta: float, alpha: float,
                 eps: float) -> torch.Tensor:
    """``out`` (2, B) f32 ← (P, nonfinite flag) of the ``B`` sequences of a time-major minibatch: ``adv`` (B·S,) the
    un-normalised advantages, ``vt`` (B·S, 4) with the valid flag in column 2. GPU only (the CPU form is
    :func:`priority_from_advantages`)."""
    from . import require
    require().seq_priority(adv, vt, out, int(B), int(S), float(eta), float(alpha), float(eps))
    return out


def scatter_priorities(priority: torch.Tensor, idx: torch.Tensor, pf: torch.Tensor, nonfinite: torch.Tensor):
    """``priority[idx[b]] = pf[0, b]`` and ``nonfinite += Σ pf[1]``, in stream order (duplicate indices of one
    minibatch carry equal values)."""
    if priority.is_cuda:
        from . import require
        require().priority_scatter(priority, idx, pf, nonfinite)
    else:
        priority.index_copy_(0, idx.to(torch.long), pf[0].to(priority.dtype))
        nonfinite += pf[1].sum().to(nonfinite.dtype)
