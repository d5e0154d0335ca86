"""Cost of the prioritised replay at the bench shape (profiles/replay_prioritized.md): one process = one variant,
prints one JSON line. Run the step variants interleaved, several times each.

    python scripts/bench_replay_priority.py <variant> [<tree>]
    variant: parent | uniform | mixture | mixture_beta | kernels

``parent`` is ``uniform`` on another source tree (``<tree>``: a checkout of the commit to compare against, with the
built libraries in place; ``mixture`` with a ``<tree>`` is the mixture sampler on that tree); ``mixture_beta`` adds the
importance-sampling weights at beta = 0.5 (profiles/replay_is_weights.md); ``kernels`` times the sampler launches alone,
without and with the weights (under rocprofv3 --kernel-trace for the per-kernel times)."""
import json
import os
import sys
import time

variant = sys.argv[1]
tree = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)

import torch  # noqa: E402

from dotaclient_amd import ops  # noqa: E402
from dotaclient_amd.learner.engine import Learner, LossConfig  # noqa: E402
from dotaclient_amd.learner.replay import HbmReplay  # noqa: E402
from dotaclient_amd.learner.synthetic import make_batch  # noqa: E402
from dotaclient_amd.models.policy import Policy, get_config  # noqa: E402

ops.require()
dev = 'cuda'
B, S, CAP = 8, 1400, 16384


def ev_time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


if variant == 'kernels':
    from dotaclient_amd.ops import replay as R
    out = {'variant': 'kernels'}
    for cap in (16384, 81920, 1 << 20):
        pri = torch.rand(cap, device=dev) + 0.01
        ver = torch.zeros(cap, dtype=torch.long, device=dev)
        st = R.SamplerState(cap, dev, seed=1)
        idx = torch.empty(B, dtype=torch.long, device=dev)
        f = lambda: R.sample_mixture(pri, ver, st, idx, cap, 0, 4096, 0.5)  # noqa: E731
        ev_time(f, 50)
        out[f'sampler_pair_us_cap{cap}'] = [round(1e3 * ev_time(f, 500), 2) for _ in range(5)]
        if hasattr(st, 'is_weight'):
            f = lambda: R.sample_mixture(pri, ver, st, idx, cap, 0, 4096, 0.5, beta=0.5,  # noqa: E731
                                         w_out=st.is_weight)
            ev_time(f, 50)
            out[f'sampler_pair_beta_us_cap{cap}'] = [round(1e3 * ev_time(f, 500), 2) for _ in range(5)]
    adv = torch.randn(B * S, device=dev)
    vt = torch.ones(B * S, 4, device=dev)
    o = torch.empty(2, B, device=dev)
    f = lambda: R.seq_priority(adv, vt, o, B, S, 0.9, 0.6, 1e-3)  # noqa: E731
    ev_time(f, 50)
    out['seq_priority_us'] = [round(1e3 * ev_time(f, 500), 2) for _ in range(5)]
    print(json.dumps(out), flush=True)
    sys.exit(0)

torch.manual_seed(7)
cfg = get_config('lstm512')
L = Learner(Policy(cfg), LossConfig(algo='ppo', vtrace=True), device=dev, backend='fused', precision='fp32-exact')
L.enable_graph(warmup=1)
mixture = variant in ('mixture', 'mixture_beta')
kw = dict(prioritized=True, sampler='mixture', recent_frac=0.5) if mixture else {}
if variant == 'mixture_beta':
    kw['priority_beta'] = 0.5
rep = HbmReplay(CAP, S, cfg.layout, cfg.hidden, dev, seed=0, vtrace=True, **kw)
rep.host_sampling = True
b = make_batch(64, S, cfg.layout, cfg.hidden, device=dev, seed=3)
g = torch.Generator(device=dev).manual_seed(3)
valid = (b['actions'].sum(-1) > 0).float()
last = (torch.rand(64, S, device=dev, generator=g) < 0.01).float()
last[:, -1] = 1.0
b['vt'] = torch.stack([torch.randn(64, S, device=dev, generator=g) * 0.3,
                       torch.randn(64, S, device=dev, generator=g) * last, valid, last], -1).contiguous()
rep.add(b, version=1)
rep.prefill()
recent = 4096 if mixture else None
step = lambda: L.train_step_replay(rep, B, recent)  # noqa: E731
for _ in range(20):
    m = step()
torch.cuda.synchronize()
wins = []
for _ in range(3):
    t0 = time.perf_counter()
    ms = ev_time(step, 100)
    torch.cuda.synchronize()
    wins.append((round(ms, 4), round(1e3 * (time.perf_counter() - t0) / 100, 4)))
print(json.dumps({'variant': variant, 'ms_per_step_events': [w[0] for w in wins],
                  'ms_per_step_host': [w[1] for w in wins], 'loss': float(m['loss']), 'graphs': len(L.graphs),
                  'priority_max': float(rep.priority.max()) if mixture else None,
                  'is_weight_min': float(m['replay/is_weight_min']) if variant == 'mixture_beta' else None}),
      flush=True)
