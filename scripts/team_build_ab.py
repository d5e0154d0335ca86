#!/usr/bin/env python3
"""A/B of two BUILDS of the extension on the team LSTM at the learner shape (fp32 W_hh, B=8, S=1400, H=512,
time-major, folded bias): both shared objects loaded into one process, interleaved rounds, µs per call of the forward
and the backward recurrence, and a bitwise comparison of every output of the two builds.

    python scripts/team_build_ab.py path/to/parent/_C.so path/to/tree/_C.so
"""
import importlib.machinery
import importlib.util
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from dotaclient_amd.ops.lstm import team_ctl  # noqa: E402


def load(path, i):
    # (the init symbol is PyInit__C in every build: the module name must end in ._C, the package part may differ)
    name = f'dca_build_{i}._C'
    spec = importlib.util.spec_from_file_location(name, path, loader=importlib.machinery.ExtensionFileLoader(name, path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(C, xp, whh, h0, c0, err, b4, dh, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tb = [], []
    for _ in range(reps):
        ev[0].record()
        f = C.lstm_team_fwd(xp, whh, h0, c0, err, team_ctl(), False, None, True, None, None, None, b4, False)
        ev[1].record()
        b = C.lstm_team_bwd(dh, f[3], f[2], c0, None, None, whh, err, team_ctl(), None, True, None, False, True, False)
        ev[2].record()
        torch.cuda.synchronize()
        tf.append(ev[0].elapsed_time(ev[1]) * 1e3)
        tb.append(ev[1].elapsed_time(ev[2]) * 1e3)
    return f, b, tf, tb


def main():
    paths = sys.argv[1:3]
    mods = [load(p, i) for i, p in enumerate(paths)]
    B, S, H = 8, 1400, 512
    torch.manual_seed(0)
    dev = 'cuda'
    xp = torch.randn(S, B, H, 4, device=dev) * 0.5
    whh = torch.randn(4 * H, H, device=dev) * 0.05
    h0 = torch.randn(B, H, device=dev) * 0.1
    c0 = torch.randn(B, H, device=dev) * 0.1
    b4 = torch.randn(4 * H, device=dev) * 0.1
    dh = torch.randn(S, B, H, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    res = [([], []) for _ in mods]
    outs = [None, None]
    for rnd in range(8):
        for i, C in enumerate(mods):
            f, b, tf, tb = run(C, xp, whh, h0, c0, err, b4, dh, 3)
            if rnd > 0:
                res[i][0].extend(tf)
                res[i][1].extend(tb)
            outs[i] = [t.clone() for t in list(f) + list(b) if t is not None and t.numel() > 0]
    for p, (f, b) in zip(paths, res):
        print(json.dumps({'build': p, 'fwd_us_median': float(np.median(f)), 'fwd_us_min': min(f), 'fwd_us_max': max(f),
                          'bwd_us_median': float(np.median(b)), 'bwd_us_min': min(b), 'bwd_us_max': max(b)}),
              flush=True)
    same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    print(json.dumps({'bitwise_equal': bool(same), 'tensors': len(outs[0]), 'err': int(err.item())}), flush=True)


if __name__ == '__main__':
    main()
