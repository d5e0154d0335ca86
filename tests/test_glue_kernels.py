"""The learner step's small glue kernels directly against float64, at the sizes where their loops change shape:
``loss_assemble`` / ``loss_prep`` / ``enc_small_grads`` (+ ``enc_small_reduce``) (ops/csrc/glue.hip), ``adv_normalize``
(ingest.hip), ``multi_axpy`` / ``multi_copy`` and the ``skip`` / no-clip flags of ``adam_step`` (adam.hip).

They are sums and element-wise maps, so wherever the inputs can be chosen so that every partial result is exactly
representable in fp32 (small integers, dyadic fractions) the kernel must equal the float64 result exactly: a row
skipped by an unrolled loop's tail or a partial dropped by a reduction tree then shows without any tolerance. Random
inputs are held to bounds derived from the fp32 format: 1e-5 × the float64 sum of the |terms| entering an output for
plain sums, and max(floor, 2 × the error of the same formulas evaluated by torch in fp32) for the gradient reductions
(the rule of tests/test_exact_row_kernels.py)."""
import functools

import pytest
import torch

from dotaclient_amd.constants import LAYOUT_1V1, LAYOUT_5V5


def _rel(a, b):
    return ((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---- loss_assemble ---------------------------------------------------------------------------------------------------
ASSEMBLE_ROWS = [1, 63, 64, 65, 447, 448, 449, 511, 512, 513, 1025, 2800]


def _assemble64(p, nrm, N, algo, ent_coef, vf_coef, S, vbug, magnitude=False):
    """The 12 outputs from the column sums p (16) in float64 — the formulas of ops/heads.py::assemble_loss (algo 2, the
    truncated-IS off-policy objective, follows the PPO branch). magnitude=True: p holds the column sums of |part| and
    every term enters with its absolute value: the size against which an fp32 evaluation's error is measured."""
    sg = 1.0 if magnitude else -1.0
    if magnitude:
        nrm = nrm.abs()
    eh = p[2:6] * nrm[2:6]
    ent = eh.sum()
    zero = torch.zeros((), dtype=torch.float64)
    kl = cf = zero
    if algo != 1:
        pol, val, entl = sg * p[0] * nrm[0], vf_coef * p[1] * nrm[0], sg * ent_coef * ent
        adv, kl, cf = p[8] * nrm[0], p[6] * nrm[0], p[7] * nrm[0]
    else:
        pol = p[0] * nrm[1]
        entl = sg * ent_coef * ent if ent_coef > 0 else zero
        val = vf_coef * p[1] / N if vf_coef > 0 else zero
        adv = p[8] / N
        if vbug and vf_coef > 0 and S > 0:
            B = N // S
            val = vf_coef * (S * p[10] + sg * 2 * p[9] * nrm[6] + N * nrm[7]) / (B * S * S)
            adv = p[9] / N + sg * nrm[6] / S
    return torch.stack([pol + val + entl, pol, entl, val, ent, adv, kl, cf, *eh])


ASSEMBLE_MODES = [(0, False), (1, False), (1, True), (2, False)]


def _run_assemble(C, part, norms, N, algo, ent_coef, vf_coef, S, vbug):
    out = torch.full((16,), 7.0, device='cuda')
    C.loss_assemble(part.cuda(), norms.cuda(), N, algo, ent_coef, vf_coef, out, S, vbug)
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[12:16] == 0).all()
    return out[:12]


@pytest.mark.parametrize('R', ASSEMBLE_ROWS)
@pytest.mark.gpu
def test_loss_assemble_exact(gpu_ops, R):
    """Small signed integers in `part`, all normalisers 1, both coefficients 1, N = 1024 and S = 4 (every division is
    by a power of two ≤ 2^11 and every output stays below 2^13, so each fp32 operation is exact): the twelve outputs
    equal the float64 values exactly, whatever rows the 8×64-row unrolled loop, its 64-row tail and the 64-group tree
    give to whom."""
    g = torch.Generator().manual_seed(R)
    part = torch.randint(-4, 5, (R, 16), generator=g).float()
    norms = torch.ones(8)
    for algo, vbug in ASSEMBLE_MODES:
        ref = _assemble64(part.double().sum(0), norms.double(), 1024, algo, 1.0, 1.0, 4, vbug)
        assert float(ref.abs().max()) < 8192
        got = _run_assemble(gpu_ops, part, norms, 1024, algo, 1.0, 1.0, 4, vbug)
        assert torch.equal(got.double(), ref), f'R={R} algo={algo} vbug={vbug}: {(got.double() - ref).tolist()}'


@pytest.mark.parametrize('R', ASSEMBLE_ROWS)
@pytest.mark.gpu
def test_loss_assemble_matches_float64(gpu_ops, R):
    """Random partials and normalisers (norms[6:8] = ΣG, ΣG² of a sequence of returns, as the direct step fills them):
    every output within 1e-5 × the float64 sum of the |terms| entering it (≈ 50 sequential fp32 adds and a 6-level
    tree: ≈ 3e-6 of that sum in the worst case)."""
    g = torch.Generator().manual_seed(100 + R)
    N, S = 1500, 50
    part = torch.randn(R, 16, generator=g)
    g_last = torch.randn(S, generator=g)
    norms = torch.cat([(torch.rand(6, generator=g) + 0.1) / N, g_last.sum().view(1), (g_last * g_last).sum().view(1)])
    worst = 0.0
    for algo, vbug in ASSEMBLE_MODES:
        ref = _assemble64(part.double().sum(0), norms.double(), N, algo, 0.01, 0.5, S, vbug)
        mag = _assemble64(part.double().abs().sum(0), norms.double(), N, algo, 0.01, 0.5, S, vbug, magnitude=True)
        got = _run_assemble(gpu_ops, part, norms, N, algo, 0.01, 0.5, S, vbug)
        err = ((got.double() - ref).abs() / mag.clamp_min(1e-300))
        err = torch.where(mag > 0, err, (got.double() - ref).abs())
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= 1e-5, f'R={R} algo={algo} vbug={vbug}: {err.tolist()}'
    print(f'loss_assemble R={R}: worst |err| / sum|terms| = {worst:.3e} (bound 1e-05)')


# ---- loss_prep -------------------------------------------------------------------------------------------------------
def _onehot_rows(N, A, gen, zero_frac=0.1, target_lo=0):
    """Hierarchical one-hot action rows as learner/synthetic.py builds them: the enum, then x and y for a move or the
    target unit for an attack; a fraction of all-zero (padded) rows. target_lo: first target slot that may be chosen."""
    U = A - 21
    act = torch.zeros(N, A, dtype=torch.uint8)
    enum = torch.randint(0, 3, (N,), generator=gen)
    if target_lo:
        enum[:] = 2
    rows = torch.arange(N)
    act[rows, enum] = 1
    move, att = enum == 1, enum == 2
    xs, ys = torch.randint(0, 9, (N,), generator=gen), torch.randint(0, 9, (N,), generator=gen)
    tgt = torch.randint(target_lo, U, (N,), generator=gen)
    act[rows[move], 3 + xs[move]] = 1
    act[rows[move], 12 + ys[move]] = 1
    act[rows[att], 21 + tgt[att]] = 1
    act[torch.rand(N, generator=gen) < zero_frac] = 0
    return act


def _check_loss_prep(C, act):
    from dotaclient_amd.ops.heads import batch_norms
    ref = batch_norms(act, torch.zeros(1), False, 1)
    ws = torch.zeros(int(C.loss_prep_ws_elems()), dtype=torch.int32, device='cuda')
    out = torch.full((8,), 7.0, device='cuda')
    dev = act.cuda()
    for _ in range(3):                           # one workspace: the arrival counter resets itself
        out.fill_(7.0)
        C.loss_prep(dev, ws, out)
        torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=0)
        assert float(out[6]) == 0.0 and float(out[7]) == 0.0
    assert int(ws[-1]) == 0
    return ref


@pytest.mark.parametrize('A', [22, 61, 85, 128])
@pytest.mark.gpu
def test_loss_prep_matches_batch_norms(gpu_ops, A):
    """Every action width (one target slot, the 1v1 layout, the 5v5 layout whose target columns pass lane 64, the widest
    row) at row counts around the 1024-wave grid; all-zero rows mixed in; every row zero (all normalisers 0)."""
    for N in (1, 4, 1023, 1024, 1025, 3000):
        g = torch.Generator().manual_seed(A * 10000 + N)
        act = _onehot_rows(N, A, g, zero_frac=0.0 if N == 1 else 0.1)
        ref = _check_loss_prep(gpu_ops, act)
        assert float(ref[0]) > 0
        zero = _check_loss_prep(gpu_ops, torch.zeros(N, A, dtype=torch.uint8))
        assert (zero == 0).all()


@pytest.mark.parametrize('A', [85, 128])
@pytest.mark.gpu
def test_loss_prep_targets_beyond_column_64(gpu_ops, A):
    """Every row an attack whose target sits in columns ≥ 64 only: the second ballot alone carries the target counts
    and the rows' validity beyond the enum."""
    for N in (4, 1025):
        g = torch.Generator().manual_seed(A + N)
        act = _onehot_rows(N, A, g, target_lo=64 - 21)
        assert int(act[:, 21:64].sum()) == 0 and int(act[:, 64:].sum()) > 0
        _check_loss_prep(gpu_ops, act)
        act[:, :3] = 0                           # rows valid through a column ≥ 64 alone
        _check_loss_prep(gpu_ops, act)


# ---- enc_small_grads + enc_small_reduce ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _enc_case(N, five):
    """env, W_env, b_env: multiples of 1/16 in [−2, 2], so the ReLU pre-activation is exact in fp32 in any order and
    the mask agrees with float64 by construction (an exact zero masks to 0 in both)."""
    layout = LAYOUT_5V5 if five else LAYOUT_1V1
    U = layout.max_units
    g = torch.Generator().manual_seed(N * 2 + int(five))
    dy = lambda *s: torch.randint(-32, 33, s, generator=g).float() / 16
    c = {'env': dy(N, 3), 'we': dy(128, 3), 'be': dy(128), 'z': torch.randn(N, 256, generator=g),
         'dtl': torch.randn(N, U, generator=g), 'dx': torch.randn(N, 896, generator=g),
         'toff': torch.tensor([0] + list(layout.offsets[1:]) + [U], dtype=torch.int32)}
    return c


def _enc_small_formulas(c, compat, dt):
    """The formulas of the kernel's header comment in dtype dt."""
    q, dtl, dx, env = c['z'][:, :128].to(dt), c['dtl'].to(dt), c['dx'].to(dt), c['env'].to(dt)
    we, be = c['we'].to(dt), c['be'].to(dt)
    off = c['toff'].tolist()
    seg = torch.stack([dtl[:, off[t]:off[t + 1]].sum(1) for t in range(6)], 1)              # (N, 6)
    pool = dx[:, 128:].reshape(-1, 6, 128).sum(0)                                           # (6, 128)
    if compat:
        pool[3] += pool[5]
        pool[5] = 0
    dbt = seg.t() @ q + pool
    de = dx[:, :128] * (env @ we.t() + be > 0).to(dt)
    return dbt, de.t() @ env, de.sum(0)


@pytest.mark.parametrize('five', [False, True], ids=['1v1', '5v5'])
@pytest.mark.parametrize('N', [1, 5, 256, 257, 8449])
@pytest.mark.gpu
def test_enc_small_grads_match_float64(gpu_ops, N, five):
    """∂b_τ, ∂W_env, ∂b_env at one row, fewer rows than blocks, one row per block, a ragged split, and more than 32 rows
    per block (the second LDS tile); both pool routings; z contiguous and as a 160-column view of 256-column rows."""
    c = _enc_case(N, five)
    dev = {k: v.cuda() for k, v in c.items()}
    for compat in (False, True):
        r64 = _enc_small_formulas(c, compat, torch.float64)
        r32 = _enc_small_formulas(c, compat, torch.float32)
        for zname, z in (('contiguous', dev['z']), ('view160', dev['z'][:, :160])):
            got = gpu_ops.enc_small_grads(z, dev['dtl'], dev['toff'], dev['dx'], dev['env'], dev['we'], dev['be'],
                                          compat)
            again = gpu_ops.enc_small_grads(z, dev['dtl'], dev['toff'], dev['dx'], dev['env'], dev['we'], dev['be'],
                                            compat)
            torch.cuda.synchronize()
            for name, a, b, e64, e32 in zip(('dbt', 'dWe', 'dbe'), got, again, r64, r32):
                assert torch.equal(a, b), f'{name} not reproducible'
                err, err32 = _rel(a, e64), _rel(e32, e64)
                print(f'enc_small_grads N={N} {"5v5" if five else "1v1"} compat={compat} {zname} {name}: {err:.3e} '
                      f'(torch fp32 {err32:.3e})')
                assert a.shape == e64.shape and err <= max(2e-6, 2 * err32), name


# ---- adv_normalize ---------------------------------------------------------------------------------------------------
def _adv_formula(adv, v, eps, dt):
    adv, v = adv.to(dt), v.to(dt)
    n = v.sum().clamp_min(1.0)
    mu = (adv * v).sum() / n
    sd = (((adv - mu) ** 2 * v).sum() / n).sqrt()
    return ((adv - mu) / (sd + eps)) * v


@pytest.mark.parametrize('L', [1, 1023, 1024, 1025, 11200])
@pytest.mark.gpu
def test_adv_normalize_matches_float64(gpu_ops, L):
    """One row per thread, the 1024-thread boundary and the strided loop beyond it; a random mask, a large mean
    (1000 + randn), no valid row (clamped count: exactly 0, finite) and exactly one valid row (exactly 0)."""
    g = torch.Generator().manual_seed(L)
    eps = 1e-8
    one = torch.zeros(L)
    one[L // 3] = 1.0
    for label, adv, v in (('random mask', torch.randn(L, generator=g) * 3 + 1, (torch.rand(L, generator=g) > 0.3).float()),
                          ('large mean', 1000 + torch.randn(L, generator=g), (torch.rand(L, generator=g) > 0.3).float()),
                          ('all invalid', 1000 + torch.randn(L, generator=g), torch.zeros(L)),
                          ('one valid', torch.randn(L, generator=g) * 3 + 1, one)):
        out = torch.full((L,), 7.0, device='cuda')
        gpu_ops.adv_normalize(adv.cuda(), v.cuda(), out, eps)
        torch.cuda.synchronize()
        out = out.cpu()
        assert torch.isfinite(out).all()
        if label in ('all invalid', 'one valid') or float(v.sum()) <= 1:
            assert (out == 0).all(), label
            continue
        ref = _adv_formula(adv, v, eps, torch.float64)
        err, err32 = _rel(out, ref), _rel(_adv_formula(adv, v, eps, torch.float32), ref)
        print(f'adv_normalize L={L} {label}: {err:.3e} (torch fp32 {err32:.3e})')
        assert err <= max(1e-6, 2 * err32), label
        assert (out[v == 0] == 0).all()


# ---- multi_axpy / multi_copy -----------------------------------------------------------------------------------------
def _axpy_sizes(n):
    if n == 1:
        return [1]
    if n == 30:                                  # a zero-element tensor in the middle and at the end
        return [1, 255, 257, 1000, 0, 64, 3] + [17 * i + 5 for i in range(22)] + [0]
    return [300, 0, 1, 2048 * 256 + 77] + [(13 * i) % 700 + 1 for i in range(59)] + [0]   # > one grid of elements


@pytest.mark.parametrize('n', [1, 30, 64])
@pytest.mark.gpu
def test_multi_axpy_matches_float64(gpu_ops, n):
    """dst_i += s·src_i over a list: scale None (= 1) and a device scalar 0.5 on dyadic data are exact, so bitwise equal
    to float64; with s = 1/3 every element is within one fp32 ulp of max(|dst|, |s·src|) of float64."""
    import numpy as np
    sizes = _axpy_sizes(n)
    assert len(sizes) == n
    g = torch.Generator().manual_seed(n)
    for scale in (None, 0.5):
        dst = [torch.randint(-64, 65, (k,), generator=g).float() / 8 for k in sizes]
        src = [torch.randint(-64, 65, (k,), generator=g).float() / 8 for k in sizes]
        dev = [d.cuda() for d in dst]
        gpu_ops.multi_axpy(dev, [s.cuda() for s in src], None if scale is None else torch.tensor([scale], device='cuda'))
        torch.cuda.synchronize()
        for i, (d, s, o) in enumerate(zip(dst, src, dev)):
            ref = d.double() + (1.0 if scale is None else scale) * s.double()
            assert torch.equal(o.cpu().double(), ref), f'tensor {i} ({sizes[i]} elements) scale={scale}'
    s32 = torch.tensor([1.0 / 3.0])
    dst = [torch.randn(k, generator=g) for k in sizes]
    src = [torch.randn(k, generator=g) for k in sizes]
    dev = [d.cuda() for d in dst]
    gpu_ops.multi_axpy(dev, [s.cuda() for s in src], s32.cuda())
    torch.cuda.synchronize()
    worst = 0.0
    for i, (d, s, o) in enumerate(zip(dst, src, dev)):
        prod = float(s32.double()) * s.double()
        ref = d.double() + prod
        ulp = torch.from_numpy(np.spacing(torch.maximum(d.double().abs(), prod.abs()).float().numpy())).double()
        ratio = (o.cpu().double() - ref).abs() / ulp
        if ratio.numel():
            worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), f'tensor {i}: {float(ratio.max()):.3f} ulp'
    print(f'multi_axpy n={n} scale=1/3: worst error {worst:.3f} ulp of max(|dst|, |s*src|) (bound 1)')


@pytest.mark.gpu
def test_multi_axpy_rejects_more_than_64_tensors(gpu_ops):
    t = [torch.zeros(4, device='cuda') for _ in range(65)]
    with pytest.raises(RuntimeError):
        gpu_ops.multi_axpy(t, [torch.ones(4, device='cuda') for _ in range(65)], None)
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0 for x in t)


@pytest.mark.gpu
def test_multi_copy_zero_byte_segments(gpu_ops):
    """A zero-byte segment in the middle of the list and at its end moves nothing and shifts no other segment."""
    g = torch.Generator().manual_seed(0)
    srcs = [torch.randn(257, generator=g), torch.empty(0), torch.randint(0, 255, (333, 61), dtype=torch.uint8, generator=g),
            torch.randn(1, generator=g), torch.empty(0, dtype=torch.uint8)]
    srcs = [s.cuda() for s in srcs]
    dsts = [torch.full_like(t, 7) for t in srcs]
    gpu_ops.multi_copy(dsts, srcs)
    torch.cuda.synchronize()
    for d, s in zip(dsts, srcs):
        assert torch.equal(d, s)


# ---- adam_step flags -------------------------------------------------------------------------------------------------
def _adam_pair(max_norm_kernel, max_norm_ref):
    from dotaclient_amd.learner.optim import FlatAdam
    from dotaclient_amd.models.policy import Policy
    from dotaclient_amd.parallel.dp import FlatParams
    torch.manual_seed(0)
    a, b = Policy('lstm128'), Policy('lstm128')
    b.load_state_dict(a.state_dict())
    fa, fb = FlatParams(a, device='cpu'), FlatParams(b.to('cuda'), device='cuda')
    oa = FlatAdam(fa, lr=1e-3, max_grad_norm=max_norm_ref, use_kernels=False)
    ob = FlatAdam(fb, lr=1e-3, max_grad_norm=max_norm_kernel, use_kernels=True)
    return fa, oa, fb, ob


def _adam_grads(fa, fb, seed):
    g = torch.Generator().manual_seed(seed)
    fa.zero_grad()
    fb.zero_grad()
    for i, (pa, pb) in enumerate(zip(fa.params, fb.params)):
        gr = torch.randn(pa.shape, generator=g) * (0.5 + i % 3)
        pa.grad.copy_(gr)
        pb.grad.copy_(gr.cuda())


@pytest.mark.gpu
def test_adam_step_skip_flag_changes_nothing(gpu_ops):
    """skip = [1.0] after a normal step (so the moments are not zero): parameters, both moments and the step counters
    stay bitwise unchanged, the gradient norm is still reported, and the non-finite flag stays clear."""
    fa, oa, fb, ob = _adam_pair(0.5, 0.5)
    _adam_grads(fa, fb, 1)
    oa.step()
    ob.step()
    before = [t.clone() for t in (fb.flat, ob.exp_avg, ob.exp_avg_sq, ob.steps)]
    assert float(ob.steps.sum()) > 0 and float(ob.exp_avg.abs().sum()) > 0
    _adam_grads(fa, fb, 2)
    oa.step(skip=torch.ones(1))
    ob.step(skip=torch.ones(1, device='cuda'))
    torch.cuda.synchronize()
    for name, x, y in zip(('params', 'exp_avg', 'exp_avg_sq', 'steps'), before,
                          (fb.flat, ob.exp_avg, ob.exp_avg_sq, ob.steps)):
        assert torch.equal(x, y), name
    torch.testing.assert_close(ob.last_grad_norm.cpu(), oa.last_grad_norm, rtol=1e-5, atol=0)
    assert float(ob.last_grad_norm) > 1.0 and float(ob.nonfinite) == 0.0
    # and the flag 0.0 applies the step
    oa.step(skip=torch.zeros(1))
    ob.step(skip=torch.zeros(1, device='cuda'))
    assert torch.equal(ob.steps, before[3] + 1)
    torch.testing.assert_close(fb.flat.cpu(), fa.flat, rtol=1e-5, atol=2e-6)


@pytest.mark.gpu
def test_adam_step_max_norm_zero_is_no_clipping(gpu_ops):
    """max_grad_norm = 0 switches the clip off (the kernel's coefficient stays 1): the update equals the reference
    without clipping, and differs from the clipped one."""
    fa, oa, fb, ob = _adam_pair(0.0, None)
    for seed in (1, 2):
        _adam_grads(fa, fb, seed)
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert float(ob.last_grad_norm) > 1.0
    torch.testing.assert_close(ob.last_grad_norm.cpu(), oa.last_grad_norm, rtol=1e-5, atol=0)
    torch.testing.assert_close(fb.flat.cpu(), fa.flat, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(ob.exp_avg.cpu(), oa.exp_avg, rtol=1e-5, atol=1e-7)
    # the kernel forms 1 − β2 in fp32: 1.f − 0.999f = 0.00099998713, 1.29e-5 below the reference's fp32(0.001)
    torch.testing.assert_close(ob.exp_avg_sq.cpu(), oa.exp_avg_sq, rtol=2e-5, atol=0)


def test_adam_reference_max_norm_zero_is_no_clipping():
    """The torch path of FlatAdam reads max_grad_norm = 0 as the kernel does: no clipping (not a zero coefficient)."""
    from dotaclient_amd.learner.optim import FlatAdam
    from dotaclient_amd.models.policy import Policy
    from dotaclient_amd.parallel.dp import FlatParams
    flats = []
    for max_norm in (0.0, None):
        torch.manual_seed(0)
        flat = FlatParams(Policy('lstm128'), device='cpu')
        opt = FlatAdam(flat, lr=1e-3, max_grad_norm=max_norm, use_kernels=False)
        g = torch.Generator().manual_seed(1)
        flat.zero_grad()
        for p in flat.params:
            p.grad.copy_(torch.randn(p.shape, generator=g))
        start = flat.flat.clone()
        opt.step()
        assert float(opt.last_grad_norm) > 1.0 and not torch.equal(flat.flat, start)
        flats.append(flat.flat.clone())
    assert torch.equal(flats[0], flats[1])
