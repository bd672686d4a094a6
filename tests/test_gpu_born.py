"""FWIForward.born (J dv) and gauss_newton (J^T W J dv) on the HIP path against the reference's own
linearisation (tests/golden/born.npz: torch.func.jvp of the reference operator in fp64 and fp32, and its fp64
autograd adjoint; tests/golden/make_born.py).

Bars.  The Born kernel runs a different but equally valid fp32 operation order than the reference's fp32 jvp, so
its yardstick is the reference's own fp32 error against fp64, E_ref[b] per model, with the factor 4 that
tests/test_gpu_sampling.py uses for its loop bar.  The adjoint identity's bar adds the project's bar of the
gradient against the reference's autograd (rel-L2 5e-5, tests/test_gpu_fwi.py).  Everything that is a property
of the schedule or of linearity is bitwise."""
import numpy as np
import pytest
import torch

from conftest import load_golden, record_margin

pytestmark = pytest.mark.gpu

CASES = ("wrap", "tiles", "geom")
GRAD_BAR = 5e-5          # gradient vs the reference's autograd, rel-L2 (tests/test_gpu_fwi.py)


class Case:
    def __init__(self, tag, cuda):
        z = load_golden("born")
        pre = f"{tag}_ctx_"
        self.ctx = {k[len(pre):]: (z[k].item() if z[k].ndim == 0 else z[k].tolist()) for k in z.files
                    if k.startswith(pre)}
        self.tag, self.normalize, self.st = tag, bool(z[f"{tag}_normalize"]), int(z[f"{tag}_st"])
        self.v = torch.from_numpy(z[f"{tag}_v"]).to(cuda)
        self.dv = torch.from_numpy(z[f"{tag}_dv"]).to(cuda)
        self.w = torch.from_numpy(z[f"{tag}_w"]).to(cuda)
        self.jdv64 = torch.from_numpy(z[f"{tag}_jdv64"]).to(cuda)
        self.jtw64 = torch.from_numpy(z[f"{tag}_jtw64"]).to(cuda)
        self.eref = z[f"{tag}_eref"]
        self.ip = float(z[f"{tag}_ip"][0])

    def fwi(self, **kw):
        from red_diffeq.solvers.pde import FWIForward
        from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
        if self.normalize:
            kw = dict(dict(v_denorm_func=v_denormalize, s_norm_func=s_normalize_none), **kw)
        return FWIForward(dict(self.ctx), "cuda", sample_temporal=self.st, normalize=self.normalize, **kw)


@pytest.fixture(scope="module")
def cases(cuda):
    return {tag: Case(tag, cuda) for tag in CASES}


def per_model_norm(t):
    return t.double().flatten(1).norm(dim=1)


def rel_l2(a, ref):
    return (per_model_norm(a.double() - ref) / per_model_norm(ref)).cpu().numpy()


def dot(a, b):
    return float((a.double() * b.double()).sum())


def identity_bound(c, jd, w, d, g):
    """sum over models of 4 E_ref |J d| |w| + 5e-5 |d| |g|: what two exact sides may differ by when the Born
    result is within its bar of J d and the gradient within its bar of J^T w."""
    e = torch.from_numpy(c.eref).to(jd.device)
    return float((4 * e * per_model_norm(jd) * per_model_norm(w)
                  + GRAD_BAR * per_model_norm(d) * per_model_norm(g)).sum())


@pytest.mark.parametrize("tag", CASES)
def test_born_against_the_references_fp64_jvp(cuda, cases, tag):
    c = cases[tag]
    fwi = c.fwi()
    seis, ds = fwi.born(c.v, c.dv, return_seis=True)
    with torch.no_grad():
        fwd = fwi(c.v)
    fwi.check()
    assert not ds.requires_grad and ds.shape == c.jdv64.shape and ds.dtype == torch.float32
    assert torch.equal(seis, fwd)
    err = rel_l2(ds, c.jdv64)
    for b, (e, eref) in enumerate(zip(err, c.eref)):
        print(f"born vs fp64 {tag}[{b}]: rel-L2 {e:.3e}, E_ref {eref:.3e}, ratio to the bar {e / (4 * eref):.3f}")
        record_margin("born_vs_fp64_over_4Eref", f"{tag}[{b}]", e, 4 * eref)
    assert (err <= 4 * c.eref).all(), (err, c.eref)


@pytest.mark.parametrize("graphs", [True, False])
def test_schedule_independence_bitwise(cuda, cases, graphs):
    """Depths 1..4 (nt = 160 leaves a one-step tail at depth 3), 1 and 3 launch chains, both coefficient
    sources, and the plan's persistent / wide settings: one J dv, bit for bit."""
    c = cases["tiles"]
    fwi = c.fwi()
    ref = fwi.born(c.v, c.dv)                                  # the plan's defaults
    plan = fwi._plan(c.v.shape[2], c.v.shape[3], c.v.device)
    plan.set_graphs(graphs)
    for depth in (1, 2, 3, 4):
        for chains in (1, 3):
            plan.set_tuning(depth, depth, chains)
            plan.set_variant(fwd_gen_coeffs=(depth + chains) % 2 == 0)
            assert torch.equal(fwi.born(c.v, c.dv), ref), (depth, chains, graphs)
    plan.set_variant()
    plan.set_persistent(0)
    plan.set_variant(wide_chunked=False)
    assert torch.equal(fwi.born(c.v, c.dv), ref)
    one = c.fwi().born(c.v[1:2].contiguous(), c.dv[1:2].contiguous())   # model 1 alone, a plan of its own
    fwi.check()
    assert torch.equal(one[0], ref[1])


@pytest.mark.parametrize("tag", CASES)
def test_linearity_bitwise(cuda, cases, tag):
    """Scaling dv by 2 is exact through a linear fp32 recurrence, underflow apart; the prologue's power-of-two
    scale (include/red_diffeq_fwi.h) takes underflow out of it for max |dv| >= 2^-64: every recorded value, the
    tiles case's precursor far below the peak included.  A zero direction gives zeros."""
    c = cases[tag]
    fwi = c.fwi()
    ds = fwi.born(c.v, c.dv)
    assert torch.equal(fwi.born(c.v, 2 * c.dv), 2 * ds)
    assert float(ds.abs().max()) > 0
    assert torch.count_nonzero(fwi.born(c.v, torch.zeros_like(c.dv))) == 0


@pytest.mark.parametrize("tag", CASES)
def test_adjoint_identity(cuda, cases, tag):
    """<J dv, w> = <dv, J^T w>: the Born pass against the hand-written adjoint (the default one)."""
    c = cases[tag]
    fwi = c.fwi()
    vv = c.v.clone().requires_grad_(True)
    (fwi(vv) * c.w).sum().backward()
    g = vv.grad
    lhs, rhs = dot(fwi.born(c.v, c.dv), c.w), dot(c.dv, g)
    fwi.check()
    bound = identity_bound(c, c.jdv64, c.w, c.dv, c.jtw64)
    print(f"adjoint identity {tag}: lhs {lhs:.9e} rhs {rhs:.9e} fp64 {c.ip:.9e} bound {bound:.3e}")
    record_margin("born_adjoint_identity_over_bound", tag, abs(lhs - rhs), bound)
    record_margin("born_lhs_vs_fp64_over_bound", tag, abs(lhs - c.ip), bound)
    record_margin("born_rhs_vs_fp64_over_bound", tag, abs(rhs - c.ip), bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert abs(lhs - c.ip) <= bound and abs(rhs - c.ip) <= bound, (lhs, rhs, c.ip, bound)


@pytest.mark.parametrize("tag", ["tiles", "geom"])
def test_gauss_newton(cuda, cases, tag):
    c = cases[tag]
    fwi = c.fwi()

    def by_hand(weight):
        vv = c.v.clone().requires_grad_(True)
        s = fwi(vv)
        ds = fwi.born(c.v, c.dv)
        s.backward(ds if weight is None else weight * ds)
        return vv.grad
    h = fwi.gauss_newton(c.v, c.dv)
    assert h.shape == c.v.shape and not h.requires_grad
    assert torch.equal(h, by_hand(None))
    weight = (torch.rand(c.w.shape, generator=torch.Generator().manual_seed(7)) > 0.3).float().to(cuda) * 0.5
    assert torch.equal(fwi.gauss_newton(c.v, c.dv, weight=weight), by_hand(weight))
    # <du, H dv> = <J du, J dv> for a second direction
    du = (float(c.dv.abs().max()) / 3 *
          torch.randn(c.dv.shape, generator=torch.Generator().manual_seed(11))).to(cuda)
    jdu, jdv = fwi.born(c.v, du), fwi.born(c.v, c.dv)
    fwi.check()
    lhs, rhs = dot(du, h), dot(jdu, jdv)
    bound = identity_bound(c, jdu, jdv, du, h)
    print(f"gauss-newton {tag}: <du, H dv> {lhs:.9e} <J du, J dv> {rhs:.9e} bound {bound:.3e}")
    record_margin("born_gauss_newton_form_over_bound", tag, abs(lhs - rhs), bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def test_custom_denormalisation_and_shot_sharding(cuda, cases):
    c = cases["tiles"]
    ref = c.fwi().born(c.v, c.dv)
    # an affine callable that is not v_denormalize itself: chained with torch.func.jvp, physical velocities to K3
    custom = c.fwi(v_denorm_func=lambda x: (x + 1) * 1500 + 1500)
    assert not custom._fused_denorm()
    err = rel_l2(custom.born(c.v, c.dv), c.jdv64)
    for b, (e, eref) in enumerate(zip(err, c.eref)):
        record_margin("born_custom_denorm_vs_fp64_over_4Eref", f"tiles[{b}]", e, 4 * eref)
    assert (err <= 4 * c.eref).all(), (err, c.eref)
    h = custom.gauss_newton(c.v, c.dv)
    assert h.shape == c.v.shape
    part = c.fwi(shots=(1, 3)).born(c.v, c.dv)
    assert torch.equal(part, ref[:, 1:3])


def test_history_budget_is_enforced(cuda, cases):
    c = cases["tiles"]
    fwi = c.fwi(history_budget_gb=1e-4)
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        fwi.born(c.v, c.dv)
