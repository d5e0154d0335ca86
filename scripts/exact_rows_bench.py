#!/usr/bin/env python
"""Per-call time of the exact team recurrence with the rows per chain forced (``team_fwd`` / ``team_bwd`` with
``exact=True, rows=r``): the A/B behind the fp32-exact plan for more than 32 sequences (profiles/exact_big_batch.md).

One process measures ONE shape; the forms alternate inside it (run 1: every form, run 2: every form, ...), each run the
median of ``--calls`` forward and of ``--calls`` backward calls timed with device events after ``--warmup`` pairs. The
error word is checked after every run and a non-zero word ends the process with exit status 3. Prints one JSON line.

Several shapes are separate processes, each under its own time limit, chained so that nothing starts after a failure:

    timeout -k 10 240 python scripts/exact_rows_bench.py --batch 64 --seq-len 1400 --rows 4,8 && \\
    timeout -k 10 120 python scripts/exact_rows_bench.py --batch 64 --seq-len 350 --rows 4,8 && \\
    timeout -k 10 120 python scripts/exact_rows_bench.py --batch 40 --seq-len 1400 --rows 4,8
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--seq-len', type=int, default=1400)
    ap.add_argument('--hidden', type=int, default=512)
    ap.add_argument('--rows', default='4,8', help='comma-separated rows per chain to compare (0 = the default plan)')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    from dotaclient_amd import ops
    from dotaclient_amd.ops.lstm import team_bwd, team_fwd, team_plan
    C = ops.require()
    B, S, H = a.batch, a.seq_len, a.hidden
    forms = [int(r) for r in a.rows.split(',')]
    g = torch.Generator(device='cuda').manual_seed(B * 100 + S)
    xp = torch.randn(S, B, H, 4, device='cuda', generator=g) * 0.5
    bias = torch.randn(4 * H, device='cuda', generator=g) * 0.3
    whh = torch.randn(4 * H, H, device='cuda', generator=g) * (1.0 / H ** 0.5)
    h0 = torch.randn(B, H, device='cuda', generator=g) * 0.3
    c0 = torch.randn(B, H, device='cuda', generator=g) * 0.3
    dh = torch.randn(S, B, H, device='cuda', generator=g)
    hs = torch.empty(S, B, H, device='cuda')
    cs = torch.empty(S, B, H, device='cuda')
    gates = torch.empty(S, B, H, 4, device='cuda')
    dg = torch.empty(S, B, H, 4, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')

    def fwd(r):
        team_fwd(C, xp, whh, h0, c0, err, False, exact=True, rows=r, time_major=True, hs_out=hs, cs_out=cs,
                 gates_out=gates, bias4=bias)

    def bwd(r):
        team_bwd(C, dh, gates, cs, c0, None, None, whh, err, exact=True, rows=r, time_major=True, dg_out=dg,
                 want_dbias=True)

    def timed(fn, r):
        t = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(r)
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(t)

    out = {'B': B, 'S': S, 'H': H, 'calls': a.calls, 'forms': {}}
    for r in forms:
        nch, Bc = team_plan(B, True, True, rows=r)
        out['forms'][str(r)] = {'nch': nch, 'Bc': Bc, 'fwd_us': [], 'bwd_us': []}
        for _ in range(a.warmup):
            fwd(r)
            bwd(r)
    torch.cuda.synchronize()
    for _ in range(a.runs):
        for r in forms:
            f = out['forms'][str(r)]
            f['fwd_us'].append(round(timed(fwd, r), 1))
            f['bwd_us'].append(round(timed(bwd, r), 1))
            torch.cuda.synchronize()
            if int(err.item()) != 0:
                print(json.dumps(dict(out, error=int(err.item()))), flush=True)
                sys.exit(3)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
