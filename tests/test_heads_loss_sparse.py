"""heads_loss loads only the unit embeddings that can reach the result (units whose target-head mask byte or action
byte is set; ops/csrc/heads_loss.hip, `need`): the outputs stay those of the dense math, and no embedding of an
unneeded (row, unit) pair is read at all.

(a) dz, dtl and logp against a float64 torch statement of the heads / loss math (learner/losses.py, the oracle of the
    fused-step tests). Bound: 1e-4 relative (norm) — fp32 rounding of the 128-term pointer dot products and of the
    softmax chain is ≈1e-7 relative per operation, the fast exp / log of the non-precise instantiation ≈1e-6; the
    fused-step tests allow 1e-3 per tensor for the whole step.
(b) a second call with every unneeded (row, unit) embedding row overwritten by NaN returns bit-identical, finite
    outputs.
(c) PPO (algo 0) and VPG (algo 1).

Row kinds (row n has kind n % 5): 0 every unit needed; 1 none (a padded step without any selection when n % 10 == 1);
2 unit 0 not needed while others are; 3 an action bit where the mask byte is 0 (inconsistent data still reads its
embedding); 4 a sparse random mask."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LDZ = 160


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _rows(N, U, g, first_kind=0):
    """actions / masks (N, 21+U) uint8 with the row kinds of the module docstring."""
    act = torch.zeros(N, 21 + U, dtype=torch.uint8)
    msk = torch.zeros(N, 21 + U, dtype=torch.uint8)
    for n in range(N):
        kind = (n + first_kind) % 5
        padded = kind == 1 and n % 10 == 1
        msk[n, 0:3] = 1
        for off in (3, 12):                                  # x / y heads: a random mask that holds the action
            m = (torch.rand(9, generator=g) < 0.6).to(torch.uint8)
            a = int(torch.randint(0, 9, (1,), generator=g))
            m[a] = 1
            msk[n, off:off + 9] = m
            if not padded and kind in (1, 4):
                act[n, off + a] = 1
        if not padded:
            act[n, int(torch.randint(0, 3, (1,), generator=g))] = 1
        t = slice(21, 21 + U)
        if kind == 0:
            msk[n, t] = 1
            act[n, 21 + int(torch.randint(0, U, (1,), generator=g))] = 1
        elif kind == 2:
            m = (torch.rand(U, generator=g) < 0.5).to(torch.uint8)
            m[0] = 0
            m[U - 1] = 1
            msk[n, t] = m
            act[n, 21 + U - 1] = 1
        elif kind == 3:
            m = (torch.rand(U, generator=g) < 0.3).to(torch.uint8)
            m[3] = 0
            m[5] = 1
            msk[n, t] = m
            act[n, 21 + 3] = 1                               # action outside the mask
        elif kind == 4:
            m = (torch.rand(U, generator=g) < 0.15).to(torch.uint8)
            a = int(torch.randint(0, U, (1,), generator=g))
            m[a] = 1
            msk[n, t] = m
            act[n, 21 + a] = 1
    return act.cuda(), msk.cuda()


def _oracle(z, emb, act, msk, adv, ret, lpo, nret, algo, U):
    from dotaclient_amd.learner.losses import head_terms, ppo_loss, split_heads, vpg_loss
    counts = {'enum': 3, 'x': 9, 'y': 9, 'target_unit': U}
    zz = z.double().requires_grad_()
    tl = torch.einsum('nd,nud->nu', zz[:, :128], emb.double())
    logits = {'enum': zz[:, 128:131], 'x': zz[:, 131:140], 'y': zz[:, 140:149], 'target_unit': tl}
    acts, msks = split_heads(act, counts), split_heads(msk, counts)
    if algo == 0:
        loss, _ = ppo_loss(logits, zz[:, 149:150], acts, msks, adv.double(), ret.double(), lpo.double(), 0.2, 0.01,
                           0.5)
    else:
        loss, _ = vpg_loss(logits, zz[:, 149:150], acts, msks, nret.double(), ret.double(), 0.01, 0.5)
    dz, dtl = torch.autograd.grad(loss, [zz, tl])
    logp = sum(t[1] for t in head_terms({k: v.detach() for k, v in logits.items()}, acts, msks).values())
    return dz, dtl, logp


def _check(C, N, U, precise, algo, first_kind=0):
    from dotaclient_amd.ops.heads import batch_norms
    g = torch.Generator().manual_seed(1000 * N + 10 * U + first_kind)
    act, msk = _rows(N, U, g, first_kind)
    z = torch.randn(N, LDZ, generator=g).cuda()
    emb = (torch.randn(N, U, 128, generator=g) * 0.1).cuda()
    adv = torch.randn(N, generator=g).cuda()
    ret = torch.randn(N, generator=g).cuda()
    nret = torch.randn(N, generator=g).cuda()
    zero = torch.zeros(N, device='cuda')
    lp64 = _oracle(z, emb, act, msk, adv, ret, zero, nret, algo, U)[2]
    lpo = (lp64 + 0.1 * torch.randn(N, generator=g).cuda().double()).float()     # ratios around 1, some clipped
    norms = batch_norms(act, ret, False, N)

    def run(e):
        return C.heads_loss(z, e, act, msk, adv, ret, lpo, nret, norms, algo, False, N, 1, 0.2, 0.01, 0.5,
                            dz_bf16=False, precise=precise)

    dz, dtl, part, lp = run(emb)
    rdz, rdtl, rlp = _oracle(z, emb, act, msk, adv, ret, lpo, nret, algo, U)
    torch.cuda.synchronize()
    e_dz, e_dtl = _rel(dz[:, :150], rdz[:, :150]), _rel(dtl, rdtl)
    e_lp = float((lp.double() - rlp).abs().max() / rlp.abs().max().clamp_min(1.0))
    print(f'N={N} U={U} precise={precise} algo={algo} kind0={first_kind}: dz {e_dz:.2e} dtl {e_dtl:.2e} logp {e_lp:.2e}')
    assert e_lp < 1e-4, e_lp
    if rdz.norm() > 0:
        assert e_dz < 1e-4, e_dz
    if rdtl.norm() > 0:
        assert e_dtl < 1e-4, e_dtl
    assert float(dz[:, 150:].abs().max()) == 0.0             # padding columns
    # (b) unneeded embeddings are never read
    unneeded = (msk[:, 21:] == 0) & (act[:, 21:] == 0)
    poisoned = emb.clone()
    poisoned[unneeded] = float('nan')
    out2 = run(poisoned)
    torch.cuda.synchronize()
    for a, b, name in zip((dz, dtl, part, lp), out2, ('dz', 'dtl', 'part', 'logp')):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    return int(unneeded.sum()), int(unneeded.numel())


@pytest.mark.parametrize('algo', [0, 1])
@pytest.mark.parametrize('precise', [True, False])
@pytest.mark.parametrize('U', [40, 64])
@pytest.mark.parametrize('N', [1, 7, 64])
def test_heads_loss_sparse_embeddings(gpu_ops, N, U, precise, algo):
    if N == 1:                                               # one row: each of the required kinds in turn
        for k in range(4):
            _check(gpu_ops, N, U, precise, algo, first_kind=k)
    else:
        skipped, total = _check(gpu_ops, N, U, precise, algo)
        assert 0 < skipped < total
