"""CPU checks of tests/xent_x16_probes.py: the builders are exact, the fp64
references agree with torch autograd, the numpy model of launch A meets every
bound tests/test_gpu_xent_x16_edges.py applies, and each of its mutants -- a
split product left out of the logits, a softmax that is wrong in one of the
ways the re-laid epilogue could be -- fails a named case under those same
bounds.  No GPU, no native library."""
import numpy as np
import pytest
import torch

import classifier_probes_x16 as p16
import xent_x16_probes as xp
from adam_ref import FLOOR

F_ = torch.nn.functional
DT = pytest.mark.parametrize("dtype", xp.DTYPES, ids=["bf16", "fp16"])
PAST = xp.past_workgroups()  # an MI355X's


def single_cases():
    out = []
    for (M, K, C, r0) in xp.SINGLE_TERM_CASES:
        M = PAST if M is None else M
        out.append((M, K, C, M - 64 if r0 is None else r0))
    return out


def single_probe(case, dtype):
    return xp.single_term_step(*case, xp.single_term_seed(*case), dtype)


def edge_cases():
    return [(M, C) for M in (7, 1000, PAST) for C in (1, 3, 17, 41, 48)]


def autograd64(X, W, b, y):
    """(loss, dW, db, G) of mean cross-entropy by torch autograd in fp64."""
    W64 = W.double().requires_grad_()
    b64 = (torch.zeros(W.shape[0]) if b is None else b).double().requires_grad_()
    z = F_.linear(X.double(), W64, b64)
    z.retain_grad()
    loss = F_.cross_entropy(z, y)
    loss.backward()
    return loss.detach(), W64.grad, b64.grad, z.grad


# ---- the builders ---------------------------------------------------------------

@DT
@pytest.mark.parametrize("case", single_cases() + [xp.SMALL_C_CASE], ids=str)
def test_single_term_step_is_what_it_says(case, dtype):
    M, K, C, r0 = case
    p = single_probe(case, dtype)
    n = min(K, M - r0)
    assert p.X.dtype == dtype and p.X.shape == (M, K) and p.n == n
    Xf = p.X.float()
    assert torch.equal(Xf.to(dtype), p.X)  # (trivially) and the values are what x says
    assert torch.equal(Xf[p.rows, p.cols].double(), p.x)
    # one element per window row, none elsewhere, every window column hit once
    nz = (Xf != 0).sum(1)
    inside = torch.zeros(M, dtype=torch.bool)
    inside[r0:r0 + n] = True
    assert torch.equal(nz, inside.long())
    assert len(set(p.cols.tolist())) == n and (Xf != 0).sum(0).max() == 1
    # full mantissas in the ranges the docstring gives
    raw = p.X[p.rows, p.cols].view(torch.int16).to(torch.int32) & 0xFFFF
    assert (raw & 1).eq(1).all()  # the lowest of the 7 / 10 mantissa bits
    assert (p.x.abs() >= 1).all() and (p.x.abs() < 4).all()
    assert (p.W.abs() >= 0.5).all() and (p.W.abs() < 4).all()
    assert (p.W.view(torch.int32) & 1).eq(1).all()
    if dtype == torch.float16:
        assert (p16.x_pieces(p.x.float().numpy(), dtype)["m"] != 0).all()
    # the logits are single products, and the labels cycle largest / smallest / random
    z = F_.linear(Xf.double(), p.W.double())
    assert torch.equal(z[p.rows], p.z64) and (z[~inside] == 0).all()
    i = torch.arange(n)
    yw = p.y[p.rows]
    assert torch.equal(yw[i % 3 == 0], p.z64.argmax(1)[i % 3 == 0])
    assert torch.equal(yw[i % 3 == 1], p.z64.argmin(1)[i % 3 == 1])
    assert int(p.y.min()) >= 0 and int(p.y.max()) < C
    # the references against autograd in fp64
    loss, dW, db, G = autograd64(p.X, p.W, None, p.y)
    torch.testing.assert_close(p.loss64, loss, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(p.db64, db, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(p.G64, M * G[p.rows], rtol=1e-12, atol=1e-15)
    # the error measure reads G back from an exact dW (and sees a stray element)
    e, stray = xp.single_term_error(p, dW)
    assert e <= 1e-12 and not stray
    other = [k for k in range(K) if k not in set(p.cols.tolist())]
    if other:
        dW2 = dW.clone()
        dW2[0, other[0]] = 1e-30
        assert xp.single_term_error(p, dW2)[1]
    else:
        assert n == K


@pytest.mark.parametrize("M,C", edge_cases())
def test_softmax_edge_step_is_what_it_says(M, C):
    p = xp.softmax_edge_step(M, C, xp.edge_seed(M, C))
    assert p.X.shape == (M, xp.EDGE_K) and p.W.shape == (C, xp.EDGE_K)
    for dt in xp.DTYPES:  # the amplitudes are exact in both 16-bit types
        assert torch.equal(p.X.to(dt).float(), p.X)
    assert set(p.X.unique().tolist()) <= set(xp.EDGE_AMPS)
    assert ((p.X != 0).sum(1) == (p.amp != 0).long()).all()
    assert ((p.W[:, 8:] != 0).sum(0) == 1).all() and (p.W[:, 8:].sum(0) == 1).all()
    for off in xp.OFFSETS:
        c = xp.edge_case(p, off)
        # the claimed fp32 logits: fl(a W + b) is what fp32 arithmetic gives, and
        # within half an ulp of the exact sum
        z64 = F_.linear(p.X.double(), p.W.double(), c.b.double())
        assert torch.equal(c.z32, (p.X @ p.W.t() + c.b))
        assert ((c.z32.double() - z64).abs() <= 2.0 ** -24 * z64.abs()).all()
        if off == 0.0:
            assert torch.equal(c.z32.double(), z64)
        # spread rows: the label on the leading class or on the smallest logit
        spread = (p.kind == 2) | (p.kind == 3)
        m = torch.arange(M)
        zk = c.z32.double()
        assert torch.equal(c.y[spread & (m % 2 == 0)], zk.argmax(1)[spread & (m % 2 == 0)])
        assert torch.equal(c.y[spread & (m % 2 == 1)], zk.argmin(1)[spread & (m % 2 == 1)])
        lead = xp.edge_case(p, off, labels="lead")
        assert torch.equal(lead.y[spread], zk.argmax(1)[spread])
        assert torch.equal(lead.y[~spread], c.y[~spread]) and torch.equal(lead.z32, c.z32)
        assert float(lead.loss) <= 10.0  # of order 1: no row pays for a lead
        if C > 1:
            lead = (zk.max(1).values - zk.median(1).values)[spread]
            assert (lead >= 255).all()
        assert (zk[p.kind == 4] == off).all()
        # the reference against autograd in fp64 on exactly those logits
        zr = zk.clone().requires_grad_()
        loss = F_.cross_entropy(zr, c.y)
        loss.backward()
        assert torch.equal(c.loss, loss.detach())
        torch.testing.assert_close(c.G, zr.grad, rtol=1e-12, atol=1e-18)
        torch.testing.assert_close(c.db, zr.grad.sum(0), rtol=1e-12, atol=1e-18)
        torch.testing.assert_close(c.dW, zr.grad.t() @ p.X.double(), rtol=1e-12, atol=1e-18)
        assert torch.isfinite(c.loss) and torch.isfinite(c.G).all()
    nb = xp.edge_case(p, 0.0, bias=False)
    assert nb.b is None and torch.equal(nb.z32, xp.edge_case(p, 0.0).z32)


def test_full_mantissa_x16_defaults_unchanged():
    """The optional exponent range leaves the default stream as it was."""
    for dt in xp.DTYPES:
        a = p16.full_mantissa_x16(torch.Generator().manual_seed(3), (257,), dt)
        lo, hi = (-20, 20) if dt == torch.bfloat16 else (-10, 10)
        b = p16.full_mantissa_x16(torch.Generator().manual_seed(3), (257,), dt, emin=lo, emax=hi)
        assert torch.equal(a, b)
        c = p16.full_mantissa_x16(torch.Generator().manual_seed(3), (257,), dt, emin=0, emax=2)
        assert (c.float().abs() >= 1).all() and (c.float().abs() < 4).all()
        with pytest.raises(AssertionError):
            p16.full_mantissa_x16(torch.Generator().manual_seed(3), (4,), dt, emin=-30, emax=2)


# ---- the model on the single-term probe -----------------------------------------

def model_on(p, dtype, **kw):
    """(loss, dW, db) of the model on a single-term probe (b = 0)."""
    return xp.model_step(p.X, p.W, torch.zeros(p.C), p.y, dtype, **kw)


@DT
@pytest.mark.parametrize("case", single_cases(), ids=str)
def test_single_term_model_and_product_mutants(case, dtype):
    """The intact model meets the GPU test's verdict against the model of an
    fp32 step (a once-rounded exact product, the same epilogue); every
    drop-one-product mutant stands at least MUTANT_MARGIN times above that
    bound and fails the verdict."""
    p = single_probe(case, dtype)
    e32, stray32 = xp.single_term_error(p, model_on(p, dtype, exact32=True)[1])
    assert not stray32
    bound = 2 * e32 + FLOOR
    e, bad = xp.check_single_term(p, model_on(p, dtype), e32)
    print(f"single-term model {case} {xp.IDS[dtype]}: e(x16)={e / FLOOR:.2f} "
          f"e(fp32)={e32 / FLOOR:.2f} FLOOR")
    assert bad == [] and e <= FLOOR and e32 <= FLOOR, (bad, e / FLOOR, e32 / FLOOR)
    for drop in p16.MUTANTS[dtype]:
        em, badm = xp.check_single_term(p, model_on(p, dtype, drop=drop), e32)
        print(f"single-term model {case} {xp.IDS[dtype]} without {drop}: e={em / FLOOR:.1f} FLOOR "
              f"= {em / bound:.1f} x the bound, fails {badm}")
        assert em >= xp.MUTANT_MARGIN * bound, (drop, em / FLOOR, bound / FLOOR)
        assert "e" in badm


@DT
def test_small_c_shape_claims_the_large_products_only(dtype):
    """At 16 x 16 x 3 the logits' errors reach G through few classes: only the
    hm (and, for fp16, mh) mutants clear the margin there, which is why the
    GPU cases start at 17 classes."""
    p = single_probe(xp.SMALL_C_CASE, dtype)
    e32, _ = xp.single_term_error(p, model_on(p, dtype, exact32=True)[1])
    bound = 2 * e32 + FLOOR
    e, bad = xp.check_single_term(p, model_on(p, dtype), e32)
    assert bad == [] and e <= FLOOR
    for drop in p16.MUTANTS[dtype]:
        em, _ = xp.check_single_term(p, model_on(p, dtype, drop=drop), e32)
        print(f"single-term model {xp.SMALL_C_CASE} {xp.IDS[dtype]} without {drop}: "
              f"{em / FLOOR:.1f} FLOOR = {em / bound:.1f} x the bound")
        if drop in ("hm", "mh"):
            assert em >= xp.MUTANT_MARGIN * bound, (drop, em / FLOOR)


@DT
def test_epilogue_mutants_on_the_single_term_probe(dtype):
    """The single-term probe's own view of the epilogue: the intact model is
    clean at every case (above); here each epilogue mutant that changes G or
    the loss on moderate logits is caught by it too."""
    caught = {}
    for case in single_cases():
        p = single_probe(case, dtype)
        e32, _ = xp.single_term_error(p, model_on(p, dtype, exact32=True)[1])
        for mutant in xp.EPILOGUE_MUTANTS:
            _, bad = xp.check_single_term(p, model_on(p, dtype, mutant=mutant), e32)
            if bad:
                caught.setdefault(mutant, (case, bad))
    print(f"single-term probe {xp.IDS[dtype]} catches: {caught}")
    for mutant in ("max_per_lane_group", "pad_classes_in_sum", "rows_past_M_in_loss"):
        assert mutant in caught, mutant


# ---- the model on the softmax edges ---------------------------------------------

def edge_verdicts(dtype, mutant=None, drop=None):
    """{case name: what failed} over every edge case of the GPU test."""
    out = {}
    for (M, C) in edge_cases():
        p = xp.softmax_edge_step(M, C, xp.edge_seed(M, C))
        for off, bias, labels in xp.edge_variants():
            c = xp.edge_case(p, off, bias=bias, labels=labels)
            loss, dW, db = xp.model_step(p.X.to(dtype), p.W, c.b, c.y, dtype, drop=drop,
                                         mutant=mutant)
            out[xp.edge_name(M, C, off, bias, labels, dtype)] = xp.check_edge(
                p, c, (loss, dW, db if bias else None))
    return out


@DT
def test_edge_model_is_clean(dtype):
    bad = {k: v for k, v in edge_verdicts(dtype).items() if v}
    assert bad == {}


@DT
@pytest.mark.parametrize("mutant", xp.EPILOGUE_MUTANTS)
def test_every_epilogue_mutant_fails_a_named_edge_case(mutant, dtype):
    bad = {k: v for k, v in edge_verdicts(dtype, mutant=mutant).items() if v}
    first = next(iter(bad.items()), None)
    print(f"{mutant} {xp.IDS[dtype]}: fails {len(bad)} edge cases, the first: {first}")
    assert bad, mutant
    # ... and where it should: the offsets for the two loss mutants, a padded
    # class count for the pad mutant, a ragged M for the row mutant
    if mutant == "no_max":
        assert any("offset +30000" in k and "finite" in v for k, v in bad.items())
    if mutant == "lse_then_subtract":
        # half an ulp of 30000 in a loss of order 1: the "lead" labels only (edge_case)
        assert all(v == ["loss"] and "30000 labels lead" in k for k, v in bad.items())
        assert {k.split(" offset ")[1].split()[0] for k in bad} == {"+30000", "-30000"}
    if mutant == "pad_classes_in_sum":
        assert all(" C=48 " not in k for k in bad) and any(" C=17 " in k for k in bad)
    if mutant == "rows_past_M_in_loss":
        assert all(v == ["loss"] for v in bad.values())
        assert {int(k.split("M=")[1].split()[0]) for k in bad} == {7, 1000, PAST}
    if mutant == "max_per_lane_group":
        assert all(" C=1 " not in k and " C=3 " not in k for k in bad)
        assert any(" C=41 " in k for k in bad)


def test_model_reads_the_ragged_tile_and_the_labels_as_the_kernel():
    """model_epilogue on hand-made logits: fp64 softmax within fp32 rounding,
    and the loss a mean over M rows whatever the tile padding."""
    g = torch.Generator().manual_seed(0)
    for (M, C) in ((1, 1), (5, 3), (16, 17), (33, 48)):
        z = (torch.randn((M, C), generator=g) * 3).numpy()
        y = torch.randint(0, C, (M,), generator=g)
        loss, G = xp.model_epilogue(z, y.numpy())
        zr = torch.from_numpy(z).double().requires_grad_()
        ref = F_.cross_entropy(zr, y)
        ref.backward()
        want = float(ref.detach())
        assert abs(float(loss) - want) <= 1e-6 * max(1.0, want)
        np.testing.assert_allclose(G, zr.grad.numpy(), rtol=0, atol=4e-7 / M)
