"""Launch helpers of the XCD-team persistent LSTM recurrence kernels (ops/csrc/lstm_team.h, lstm_team_fwd.hip,
lstm_team_bwd.hip).

* ``team_fwd`` — the recurrence in ONE persistent launch (``_C.lstm_team_fwd``): 32 workgroups of ONE XCD per
  sequence chain, exchanging the step state through that XCD's L2, gates in unit-major (…, H, 4) layout; it saves the
  activated gates and cell states for the backward;
* ``team_bwd`` — the reverse recurrence in one launch (``_C.lstm_team_bwd``) producing ∂L/∂gates for every step (the
  weight gradients are the learner's split-K GEMMs, ops/csrc/gemm_tn.hip);
* ``team_plan`` — how a launch splits its sequences into chains (the mirror of the launcher's plan; ``exact=True`` is
  the fp32-exact plan, which keeps every batch size on the exact VALU forms);
* ``gate_perm`` / ``team_ctl`` — the gate-major → unit-major row permutation and the per-stream control block;
* ``parse_team_stats`` / ``merge_team_stats`` — the decoder of the recurrence's telemetry block (did every XCD team
  form, how were the chains spread, how long did the call take on the device; layout below). The kernels do not write
  such a block yet (profiles/team_telemetry.md): this is the host half, which the learner's metrics are built on.

(A cross-XCD "ring" recurrence — every hand-off over the Infinity Fabric — measured 2.5-3 µs per step against the
team kernel's ≈1.3-1.5 µs and was removed in round 5. The ``nn.LSTM``-shaped autograd wrapper that tests the
kernels against torch lives in tests/test_lstm_kernel.py.)
"""
from __future__ import annotations

import numpy as np
import torch

# Layout of a statistics block: one per (device, stream) like ``team_ctl``, zero-initialised, 32-bit words, 64-bit
# values as two words (lo, hi), times in s_memrealtime ticks (100 MHz). One writer per launch (thread 0 of the last
# workgroup to exit), so no atomics.
#   word 0            seq: launches recorded on this block (= the newest record's seq), written last
#   words 8 + 16·k …  running totals of kind k (0 forward, 1 backward):
#       +0 launches   +1 launches that ended with a non-zero error word   +2 degraded launches
#       +3 teams aborted (leader timed out, state 2)   +4 teams absent (no ticket taken on that XCD)
#       +5,+6 chains run   +7,+8 tick sum   +9,+10 tick maximum
#   words 64 + 16·s … ring of the 64 most recent launches, slot s = (seq - 1) % 64, 64 bytes each:
#       +0 seq (1-based; written last, 0 = never used)   +1 kind   +2 nch   +3 the sticky error word seen at exit
#       +4 XCD masks: committed (state 1) | aborted (state 2) << 8 | absent << 16
#       +5…+8 chains run by teams 0…7, 16 bits each (team 2i in the low half of word 5 + i)
#       +9,+10 ticks from the first workgroup's arrival to the last workgroup's exit
#       +11,+12 ticks from the first arrival to the first chain being handed out
#   every other word is reserved (0).
# A launch is DEGRADED when some team ran more chains than the even spread, max_x chains[x] > ceil(nch / 8).
STAT_RING = 64
STAT_HDR_WORDS = 64
STAT_KIND_BASE = 8
STAT_KIND_WORDS = 16
STAT_REC_WORDS = 16
STAT_WORDS = STAT_HDR_WORDS + STAT_RING * STAT_REC_WORDS
STAT_KINDS = ('fwd', 'bwd')
TICKS_PER_MS = 1e5                     # s_memrealtime: 100 MHz


def gate_perm(H: int, device) -> torch.Tensor:
    """Row permutation gate-major (q·H + j) → unit-major (4·j + q): W[perm] puts a unit's 4 gates together."""
    j = torch.arange(H, device=device)
    return (torch.arange(4, device=device)[None, :] * H + j[:, None]).reshape(-1)


_CTL = {}


def team_ctl(device=None, stream=None) -> torch.Tensor:
    """The persistent, self-cleaning control block for team-LSTM launches on (device, stream): zero-initialised
    once; each launch leaves it clean for the next one and advances its epoch (lstm_team.h ``TeamCtl``). Team
    kernels on different streams must not share a block, kernels on one stream are serialised anyway."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    key = (dev.index, s.cuda_stream)
    t = _CTL.get(key)
    if t is None:
        t = _CTL[key] = torch.zeros(64, dtype=torch.int32, device=dev)
    return t


def _u64(lo, hi) -> int:
    return (int(hi) << 32) | int(lo)


def _xcds(mask: int):
    return [x for x in range(8) if (mask >> x) & 1]


def _empty_totals():
    return {'launches': 0, 'errors': 0, 'degraded': 0, 'aborted': 0, 'absent': 0, 'chains': 0, 'ticks': 0,
            'ms_sum': 0.0, 'ms_max': 0.0}


def parse_team_stats(block) -> dict:
    """Decode a HOST copy of a statistics block (numpy array or CPU tensor of ≥ ``STAT_WORDS`` 32-bit words).

    Returns ``{'seq', 'fwd': totals, 'bwd': totals, 'records': [...], 'lost'}``: the per-kind running totals
    (``launches, errors, degraded, aborted, absent, chains, ticks, ms_sum, ms_max``; times in ms = ticks / 1e5), the
    ring in launch order, oldest first (``seq, kind, nch, err, committed, aborted, absent`` — lists of XCD ids —,
    ``chains`` (8 ints), ``ticks, ms, queue_ms, degraded``) and the number of launches that fell out of the ring."""
    if isinstance(block, torch.Tensor):
        block = block.detach().cpu().contiguous().numpy()
    w = np.ascontiguousarray(block).view(np.uint32).reshape(-1)
    if w.size < STAT_WORDS:
        raise ValueError(f'statistics block too small: {w.size} words, needs {STAT_WORDS}')
    out = {'seq': int(w[0])}
    for k, name in enumerate(STAT_KINDS):
        t = w[STAT_KIND_BASE + STAT_KIND_WORDS * k:][:STAT_KIND_WORDS]
        ticks = _u64(t[7], t[8])
        out[name] = {'launches': int(t[0]), 'errors': int(t[1]), 'degraded': int(t[2]), 'aborted': int(t[3]),
                     'absent': int(t[4]), 'chains': _u64(t[5], t[6]), 'ticks': ticks,
                     'ms_sum': ticks / TICKS_PER_MS, 'ms_max': _u64(t[9], t[10]) / TICKS_PER_MS}
    recs = []
    for s in range(STAT_RING):
        r = w[STAT_HDR_WORDS + STAT_REC_WORDS * s:][:STAT_REC_WORDS]
        if int(r[0]) == 0:
            continue
        chains = [(int(r[5 + (x >> 1)]) >> (16 * (x & 1))) & 0xffff for x in range(8)]
        nch = int(r[2])
        ticks = _u64(r[9], r[10])
        recs.append({'seq': int(r[0]), 'kind': STAT_KINDS[int(r[1]) & 1], 'nch': nch, 'err': int(r[3]),
                     'committed': _xcds(int(r[4])), 'aborted': _xcds(int(r[4]) >> 8),
                     'absent': _xcds(int(r[4]) >> 16), 'chains': chains, 'ticks': ticks,
                     'ms': ticks / TICKS_PER_MS, 'queue_ms': _u64(r[11], r[12]) / TICKS_PER_MS,
                     'degraded': max(chains) > (nch + 7) // 8})
    recs.sort(key=lambda r: r['seq'])
    out['records'] = recs
    out['lost'] = out['seq'] - len(recs)
    return out


def merge_team_stats(parsed) -> dict:
    """Sum the totals of several parsed blocks (one per stream); records keep their block's index as ``block``."""
    out = {'seq': 0, 'fwd': _empty_totals(), 'bwd': _empty_totals(), 'records': [], 'lost': 0}
    for i, p in enumerate(parsed):
        out['seq'] += p['seq']
        out['lost'] += p['lost']
        for name in STAT_KINDS:
            a, b = out[name], p[name]
            for k in ('launches', 'errors', 'degraded', 'aborted', 'absent', 'chains', 'ticks'):
                a[k] += b[k]
            a['ms_sum'] = a['ticks'] / TICKS_PER_MS
            a['ms_max'] = max(a['ms_max'], b['ms_max'])
        out['records'] += [dict(r, block=i) for r in p['records']]
    return out


TEAMS = 8                              # XCD teams of a launch (lstm_team.h kMaxTeams)
EXACT_ROWS = (1, 2, 4, 8)              # rows per chain of the exact VALU forms the build dispatches
EXACT_MAX_CHAINS = 32                  # queue bound of the exact plan (lstm_team.h kMaxQueue, at make_tagbase)
EXACT_MAX_BATCH = EXACT_MAX_CHAINS * EXACT_ROWS[-1]


def team_plan(B: int, f32: bool, exact: bool, rows: int = 0):
    """``(nch, Bc)`` of a team-recurrence launch of ``B`` sequences: the pure-Python mirror of lstm_team.h
    ``plan()`` / ``plan_exact()``. Chain ``c`` holds the sequences ``[c·Bc, min((c + 1)·Bc, B))`` (empty where that
    range is); a chain of ``Bc`` rows runs the next kernel form up (1, 2, 4, 8 rows).

    ``exact`` (fp32 weights only) is the fp32-exact plan: exact VALU chains at every ``B`` — one chain per XCD team
    while ``B`` ≤ 8 × 8, then ``ceil(B / 8)`` queued chains of 8 rows, at most ``EXACT_MAX_CHAINS`` of them. ``rows``
    (only with ``exact``) forces the rows per chain. Raises ``ValueError`` for what the launcher refuses."""
    B, rows = int(B), int(rows)
    if B < 1:
        raise ValueError(f'team_plan: B = {B}')
    if not exact:
        if rows != 0:
            raise ValueError('team_plan: rows needs exact')
        nch = min(B, TEAMS) if B <= TEAMS * 32 else (B + 31) // 32
        if f32 and (B + nch - 1) // nch > 16:       # fp32 MFMA chains hold at most 16 rows
            nch = (B + 15) // 16
        return nch, (B + nch - 1) // nch
    if not f32:
        raise ValueError('team_plan: exact needs fp32 weights')
    if rows != 0 and rows not in EXACT_ROWS:
        raise ValueError(f'team_plan: rows = {rows}, not one of 0, {", ".join(map(str, EXACT_ROWS))}')
    rmax = EXACT_ROWS[-1]
    if rows != 0:
        nch, Bc = (B + rows - 1) // rows, rows
    elif B <= TEAMS * rmax:
        nch = min(B, TEAMS)
        Bc = (B + nch - 1) // nch
    else:
        nch, Bc = (B + rmax - 1) // rmax, rmax
    if nch > EXACT_MAX_CHAINS:
        raise ValueError(f'team_plan: {nch} chains of {Bc} rows for B = {B}, the exact plan queues at most '
                         f'{EXACT_MAX_CHAINS} (B ≤ {EXACT_MAX_CHAINS * (rows or rmax)})')
    return nch, Bc


def team_fwd(C, xp4, whh16, h0, c0, err, want_f32_h, exact=False, rows=0, **kw):
    return C.lstm_team_fwd(xp4, whh16, h0.contiguous(), c0.contiguous(), err, team_ctl(xp4.device), want_f32_h,
                           exact=exact, rows=rows, **kw)


def team_bwd(C, dhs, gates4, cs, c0, dhn, dcn, whh16, err, exact=False, rows=0, **kw):
    return C.lstm_team_bwd(dhs, gates4, cs, c0.contiguous(), dhn, dcn, whh16, err, team_ctl(dhs.device),
                           exact=exact, rows=rows, **kw)
