"""Encoded simultaneous-source supershots on the HIP path, FWIForward.forward(v, wavelet=W, encoding=E): the narrow
chunked kernels' ENC instantiations, the encoded finalize and the enc_fwi* operators, against
tests/golden/encoding.npz (fp64 truth from per-shot reference runs combined by linearity, and the reference's own fp32
error as the yardstick: tests/golden/make_encoding.py) and against the per-shot wavelet path forward(v, wavelet=W),
which tests/test_gpu_wavelet.py ties to the reference bit for bit.

Bars.  A supershot with one non-zero code of 1 is the per-shot path's record: bitwise (the other sources add exact
zeros), and with E = I every accumulator and gradient is the per-shot path's: bitwise.  General codes sum the sources
in one wavefield where the truth sums records, so they are held to the project's 4 x the reference's own fp32 error:
seis per (model, supershot) against 4 E_ref, W.grad and E.grad per model against 4 eref_w and 4 eref_E; dL/dv keeps
the project's 5e-5.  Everything that is a property of the schedule is bitwise, except dL/dv across settings that
change the adjoint's launches, where the sponge partials are summed in another fp64 order (1e-6, as
tests/test_gpu_wavelet.py)."""
import numpy as np
import pytest
import torch

from conftest import record_margin
from encoding_cases import CASES, Fixture

pytestmark = pytest.mark.gpu

GRAD_BAR = 5e-5          # dL/dv against the reference's autograd, rel-L2 (tests/test_gpu_wavelet.py)
GK_ORDER_BAR = 1e-6      # dL/dv between two fp64 summation orders of gk_part (tests/test_gpu_wavelet.py)


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def per_model(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).reshape(a.shape[0], -1).sum(1))


class Case(Fixture):
    def __init__(self, tag, cuda):
        super().__init__(tag)
        self.tv, self.tW, self.tE, self.tr = (torch.from_numpy(a).to(cuda) for a in (self.v, self.W, self.E, self.r))
        self.tdW = torch.from_numpy(self.dW).to(cuda)
        self._ref = None

    def gradients(self, fwi, E=None, W=None, r=None, want=(True, True, True)):
        """(seis, v.grad, W.grad, E.grad) of <fwi(v, wavelet=W, encoding=E), r>, as tensors (None where not asked
        for).  E defaults to the fixture's codes as a full (B, ne, ns) tensor, as the fixture's gE64 is laid out."""
        E = self.tE.expand(self.B, -1, -1).contiguous() if E is None else E
        v = self.tv.clone().requires_grad_(want[0])
        w = (self.tW if W is None else W).clone().requires_grad_(want[1])
        e = E.clone().requires_grad_(want[2])
        seis = fwi(v, wavelet=w, encoding=e)
        (seis * (self.tr if r is None else r)).sum().backward()
        return seis.detach(), v.grad, w.grad, e.grad

    def reference(self):
        """All the fixture's codes on a fresh operator's defaults (store-all), computed once and shared."""
        if self._ref is None:
            fwi = self.fwi()
            self._ref = self.gradients(fwi)
            fwi.check()
        return self._ref


@pytest.fixture(scope="module")
def cases(cuda):
    return {tag: Case(tag, cuda) for tag in CASES}


def accumulators(monkeypatch_target, names):
    """Record the outputs of the named adjoint ops of red_diffeq.ops while they run (the autograd backward looks
    them up by name): {name: [(gA, gk, gbeta, gw), ...]}."""
    from red_diffeq import ops as O
    seen = {n: [] for n in names}
    for n in names:
        real = getattr(O, n)

        def spy(*args, _real=real, _n=n):
            out = _real(*args)
            seen[_n].append(tuple(out))
            return out
        monkeypatch_target.setattr(O, n, spy)
    return seen


# --------------------------------------------------------------------------------------- 1. one-hot rows
@pytest.mark.parametrize("ckpt", [None, 40])
@pytest.mark.parametrize("tag", CASES)
def test_one_hot_rows_are_the_per_shot_records(cuda, cases, tag, ckpt):
    """Row e with a single 1 at source s: the record of shot s of forward(v, wavelet=W), bit for bit, in the call
    that keeps a history (or checkpoints) and in the no-grad call.  ne = 2 ns rows, each source twice."""
    c = cases[tag]
    fwi = c.fwi(checkpoint=ckpt)
    order = list(range(c.ns - 1, -1, -1)) + list(range(c.ns))
    E = torch.eye(c.ns, device=cuda)[order]
    with torch.no_grad():
        shots = fwi(c.tv, wavelet=c.tW)
        enc = fwi(c.tv, wavelet=c.tW, encoding=E)
    assert enc.shape == (c.B, 2 * c.ns) + tuple(shots.shape[2:]) and enc.dtype == torch.float32
    assert torch.equal(enc, shots[:, order]), tag
    assert float(shots.abs().max()) > 0
    v = c.tv.clone().requires_grad_(True)
    kept = fwi(v, wavelet=c.tW, encoding=E)                             # history / checkpoint pass
    assert torch.equal(kept.detach(), shots[:, order]), tag
    fwi.check()


# --------------------------------------------------------------------------------------- 2. identity code
@pytest.mark.parametrize("ckpt", [None, 40])
@pytest.mark.parametrize("tag", CASES)
def test_identity_code_is_the_per_shot_gradient(cuda, cases, tag, ckpt, monkeypatch):
    """E = I and the same upstream gradient: v.grad, W.grad and the accumulators gA, gk_part and gbeta (the diagonal
    of the encoded (B, ne, ns); off it, sums of signed zeros) are the per-shot wavelet path's, torch.equal."""
    c = cases[tag]
    names = ["fwi_adjoint_src", "enc_fwi_adjoint"] if ckpt is None else ["fwi_adjoint_ckpt_src", "enc_fwi_adjoint_ckpt"]
    seen = accumulators(monkeypatch, names)
    fwi = c.fwi(checkpoint=ckpt)
    r = c.tr[:, :1].expand(-1, c.ns, -1, -1).contiguous()
    v1, w1 = c.tv.clone().requires_grad_(True), c.tW.clone().requires_grad_(True)
    s1 = fwi(v1, wavelet=w1)
    (s1 * r).sum().backward()
    v2, w2 = c.tv.clone().requires_grad_(True), c.tW.clone().requires_grad_(True)
    E = torch.eye(c.ns, device=cuda).requires_grad_(True)
    s2 = fwi(v2, wavelet=w2, encoding=E)
    (s2 * r).sum().backward()
    fwi.check()
    assert torch.equal(s1, s2)
    assert torch.equal(v1.grad, v2.grad) and torch.equal(w1.grad, w2.grad), tag
    (gA1, gk1, gb1, gw1), = seen[names[0]]
    (gA2, gk2, gb2, gw2), = seen[names[1]]
    assert torch.equal(gA1, gA2) and torch.equal(gk1, gk2), tag
    gb2 = gb2.view(c.B, c.ns, c.ns)
    assert torch.equal(gb1.view(c.B, c.ns), gb2.diagonal(dim1=1, dim2=2)), tag
    assert torch.equal(gb1.view(c.B, c.ns), gb2.sum(1))                  # what the finalize folds
    off = gb2[:, ~torch.eye(c.ns, dtype=torch.bool, device=cuda)]
    assert torch.count_nonzero(off) == 0
    assert torch.equal(gw1, gw2.diagonal(dim1=1, dim2=2).permute(0, 2, 1)), tag
    assert E.grad.shape == (c.ns, c.ns) and float(E.grad.abs().max()) > 0


# ------------------------------------------------------------------------------ 3. general codes, forward
@pytest.mark.parametrize("tag", CASES)
def test_general_codes_forward_against_fp64(cuda, cases, tag):
    """rel-L2 per (model, supershot) against the fp64 truth <= 4 E_ref, for all the codes at once (ne = ns + 2 > ns),
    and for the sign rows, the Gaussian rows with an exact zero and ne = 1 as calls of their own, which give the
    same rows bit for bit (the supershots of a call do not interact)."""
    c = cases[tag]
    fwi = c.fwi()
    seis = c.reference()[0]
    assert seis.shape == c.seis64.shape and seis.dtype == torch.float32
    got = seis.cpu().numpy()
    worst = 0.0
    for b in range(c.B):
        for e in range(c.ne):
            err = rel_l2(got[b, e], c.seis64[b, e])
            worst = max(worst, err / (4 * c.eref[b, e]))
            print(f"seis vs fp64 {tag}[{b},{e}]: rel-L2 {err:.3e}, E_ref {c.eref[b, e]:.3e}, ratio to the bar "
                  f"{err / (4 * c.eref[b, e]):.3f}")
            record_margin("encoding_seis_vs_fp64_over_4Eref", f"{tag}[{b},{e}]", err, 4 * c.eref[b, e])
    with torch.no_grad():
        for name, rows in c.codes.items():
            part = fwi(c.tv, wavelet=c.tW, encoding=c.tE[rows])          # (ne, ns): shared by the models
            assert torch.equal(part, seis[:, rows]), (tag, name)
    fwi.check()
    assert worst <= 1.0, (tag, worst)


# ---------------------------------------------------------------------------- 4. general codes, gradients
@pytest.mark.parametrize("tag", CASES)
def test_general_codes_gradients_against_fp64(cuda, cases, tag):
    c = cases[tag]
    _, gv, gW, gE = c.reference()
    gv, gW, gE = gv.cpu().numpy(), gW.cpu().numpy(), gE.cpu().numpy()
    assert gW.shape == c.gW64.shape and gE.shape == c.gE64.shape and gv.shape == c.gv64.shape
    ev = rel_l2(gv, c.gv64)
    print(f"v.grad vs fp64 {tag}: rel-L2 {ev:.3e} (the reference's own fp32: {c.eref_v})")
    record_margin("encoding_dLdv_vs_fp64", tag, ev, GRAD_BAR)
    ok = ev <= GRAD_BAR
    for b in range(c.B):
        ew, eE = rel_l2(gW[b], c.gW64[b]), rel_l2(gE[b], c.gE64[b])
        print(f"W.grad vs fp64 {tag}[{b}]: rel-L2 {ew:.3e}, ratio to 4 eref_w {ew / (4 * c.eref_w[b]):.3f};  "
              f"E.grad: {eE:.3e}, ratio to 4 eref_E {eE / (4 * c.eref_E[b]):.3f}")
        record_margin("encoding_Wgrad_vs_fp64_over_4Eref", f"{tag}[{b}]", ew, 4 * c.eref_w[b])
        record_margin("encoding_Egrad_vs_fp64_over_4Eref", f"{tag}[{b}]", eE, 4 * c.eref_E[b])
        ok = ok and ew <= 4 * c.eref_w[b] and eE <= 4 * c.eref_E[b]
    assert ok, tag


@pytest.mark.parametrize("tag", ["tiles", "shared"])
def test_broadcast_codes_and_wavelets_receive_the_sums(cuda, cases, tag):
    """E of shape (ne, ns) receives the sum over models of the gradient the same codes get as a full (B, ne, ns)
    tensor, and a (ns, nt) wavelet the sum over models: against torch.sum of the full-shape result bit for bit, and
    against fp64 under the summed per-model bars."""
    c = cases[tag]
    fwi = c.fwi()
    _, _, _, gE_full = c.reference()
    _, _, _, gE = c.gradients(fwi, E=c.tE, want=(False, False, True))
    assert gE.shape == (c.ne, c.ns) and torch.equal(gE, gE_full.sum(0))
    bar = float((4 * c.eref_E * per_model(c.gE64)).sum())
    err = float(np.linalg.norm(gE.cpu().numpy().astype(np.float64) - c.gE64.sum(0)))
    record_margin("encoding_Egrad_shared_models_over_bound", tag, err, bar)
    assert err <= bar, (err, bar)
    # (ns, nt): model 0's wavelets for every model; the truth's gW64 does not depend on W (linear), so it sums too
    w2 = c.tW[0]
    _, _, gW, _ = c.gradients(fwi, W=w2, want=(False, True, False))
    _, _, gW_full, _ = c.gradients(fwi, W=w2.expand(c.B, -1, -1).contiguous(), want=(False, True, False))
    assert gW.shape == (c.ns, c.nt) and torch.equal(gW, gW_full.sum(0))
    bar = float((4 * c.eref_w * per_model(c.gW64)).sum())
    err = float(np.linalg.norm(gW.cpu().numpy().astype(np.float64) - c.gW64.sum(0)))
    record_margin("encoding_Wgrad_shared_models_over_bound", tag, err, bar)
    assert err <= bar, (err, bar)
    fwi.check()


# ------------------------------------------------------------------------------------- 5. the shared cell
def test_shared_cell_sources_swap(cuda, cases):
    """Sources 1 and 2 of `shared` sit on one padded cell.  Swapping their rows of W and their columns of E
    together is the same physical supershot with the two adds in the other order: the same seismograms within the
    bar of test 3 (each against the fp64 truth, which is symmetric in the two)."""
    c = cases["shared"]
    fwi = c.fwi()
    swap = [0, 2, 1]
    with torch.no_grad():
        a = fwi(c.tv, wavelet=c.tW, encoding=c.tE)
        b = fwi(c.tv, wavelet=c.tW[:, swap].contiguous(), encoding=c.tE[:, swap].contiguous())
    fwi.check()
    assert torch.equal(a, c.reference()[0])
    got = b.cpu().numpy()
    for m in range(c.B):
        for e in range(c.ne):
            err = rel_l2(got[m, e], c.seis64[m, e])
            record_margin("encoding_shared_swapped_vs_fp64_over_4Eref", f"shared[{m},{e}]", err, 4 * c.eref[m, e])
            assert err <= 4 * c.eref[m, e], (m, e, err)
    d = float((a - b).abs().max() / a.abs().max())
    print(f"shared, swapped order of the two adds: max |a - b| / max |a| = {d:.3e}")
    assert d < 1e-5


# ------------------------------------------------------------------------------- 6. schedule independence
def test_accumulators_and_gwav_across_schedules(cuda, cases, monkeypatch):
    """seis, gwav, gA and gbeta bit for bit across depths 1-4, chains {1, 2, 3}, graphs on / off and both
    coefficient sources; dL/dv bitwise at the reference's adjoint depth and within the gk_part rule elsewhere.
    Several chains run as direct launches only: capturing a graph with parallel branches is the open host fault of
    DESIGN's Born section, which tests/test_gpu_wavelet.py stays clear of in the same way; the chains' launches
    are the same either way."""
    c = cases["tiles"]
    seen = accumulators(monkeypatch, ["enc_fwi_adjoint"])
    seis0, gv0, gW0, gE0 = c.gradients(c.fwi())
    gA0, _, gb0, gw0 = seen["enc_fwi_adjoint"].pop()
    assert gw0.shape == (c.B, c.ne, c.ns, c.nt) and gb0.numel() == c.B * c.ne * c.ns
    assert torch.equal(seis0, c.reference()[0])
    fwi = c.fwi()
    plan = fwi._plan(c.tv.shape[2], c.tv.shape[3], c.tv.device)
    for graphs in (True, False):
        plan.set_graphs(graphs)
        for depth in (1, 2, 3, 4):
            for chains in ((1,) if graphs else (1, 2, 3)):
                plan.set_tuning(depth, depth, chains)
                plan.set_variant(fwd_gen_coeffs=(depth + chains) % 2 == 0)
                seis, gv, gW, gE = c.gradients(fwi)
                gA, _, gb, gw = seen["enc_fwi_adjoint"].pop()
                key = (graphs, depth, chains)
                assert torch.equal(seis, seis0) and torch.equal(gw, gw0), key
                assert torch.equal(gA, gA0) and torch.equal(gb, gb0), key
                assert torch.equal(gW, gW0) and torch.equal(gE, gE0), key
                if depth == 4:
                    assert torch.equal(gv, gv0), key
                else:
                    e = rel_l2(gv.cpu().numpy(), gv0.cpu().numpy())
                    record_margin("encoding_dLdv_across_depths", f"graphs={graphs},depth={depth},chains={chains}", e,
                                  GK_ORDER_BAR)
                    assert e < GK_ORDER_BAR, (key, e)
    fwi.check()


@pytest.mark.parametrize("K", [1, 7, 40, 160, 320])
def test_checkpointed_gradient(cuda, cases, K, monkeypatch):
    c = cases["tiles"]
    assert c.nt == 160
    seen = accumulators(monkeypatch, ["enc_fwi_adjoint", "enc_fwi_adjoint_ckpt"])
    seis0, gv0, gW0, gE0 = c.gradients(c.fwi())
    gA0, _, gb0, gw0 = seen["enc_fwi_adjoint"].pop()
    fwi = c.fwi(checkpoint=K)
    seis, gv, gW, gE = c.gradients(fwi)
    fwi.check()
    gA, _, gb, gw = seen["enc_fwi_adjoint_ckpt"].pop()
    assert torch.equal(seis, seis0) and torch.equal(gw, gw0) and torch.equal(gA, gA0) and torch.equal(gb, gb0), K
    assert torch.equal(gW, gW0) and torch.equal(gE, gE0), K
    e = rel_l2(gv.cpu().numpy(), gv0.cpu().numpy())
    record_margin("encoding_checkpoint_dLdv_vs_store_all", f"K={K}", e, GK_ORDER_BAR)
    assert e < GK_ORDER_BAR, (K, e)
    if K % 4 == 0 or K >= c.nt:
        assert torch.equal(gv, gv0), K


def test_checkpointed_short_record(cuda, cases):
    c = cases["short"]
    seis0, gv0, gW0, gE0 = c.reference()
    for K in (3, 4):
        seis, gv, gW, gE = c.gradients(c.fwi(checkpoint=K))
        assert torch.equal(seis, seis0) and torch.equal(gW, gW0) and torch.equal(gE, gE0), K
        assert rel_l2(gv.cpu().numpy(), gv0.cpu().numpy()) < GK_ORDER_BAR, K


# ------------------------------------------------------------------------------------ 7. adjoint identity
@pytest.mark.parametrize("tag", CASES)
def test_adjoint_identity(cuda, cases, tag):
    """<F_E(v, dW), r> = <dW, W.grad>, F_E(v, dW) being forward(v, wavelet=dW, encoding=E) under no_grad.  Bound, as
    tests/test_gpu_wavelet.py::test_adjoint_identity: the left side may sit 4 E_fwd |F dW| |r| from the fp64 value,
    E_fwd the reference's own fp32 forward error on this case (E_ref, the largest per model; the forward is linear in
    the wavelet, so the relative error carries over), and the right side 4 eref_w |dW| |gW64|."""
    c = cases[tag]
    fwi = c.fwi()
    with torch.no_grad():
        jdw = fwi(c.tv, wavelet=c.tdW, encoding=c.tE).cpu().numpy()
    fwi.check()
    gW = c.reference()[2].cpu().numpy()
    lhs = float((jdw.astype(np.float64) * c.r).sum())
    rhs = float((c.dW.astype(np.float64) * gW).sum())
    efwd = c.eref.max(1)
    bound = float((4 * efwd * per_model(jdw) * per_model(c.r) + 4 * c.eref_w * per_model(c.dW) * per_model(c.gW64)).sum())
    print(f"adjoint identity {tag}: lhs {lhs:.9e} rhs {rhs:.9e} fp64 {c.ip[0]:.9e} bound {bound:.3e}")
    record_margin("encoding_adjoint_identity_over_bound", tag, abs(lhs - rhs), bound)
    record_margin("encoding_lhs_vs_fp64_over_bound", tag, abs(lhs - c.ip[0]), bound)
    record_margin("encoding_rhs_vs_fp64_over_bound", tag, abs(rhs - c.ip[0]), bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert abs(lhs - c.ip[0]) <= bound and abs(rhs - c.ip[0]) <= bound, (lhs, rhs, c.ip, bound)


# ---------------------------------------------------------------------------------------------- 8. ops
def test_ops_opcheck(cuda, cases):
    from torch.library import opcheck
    c = cases["wrap"]
    fwi = c.fwi()
    plan = fwi._plan(c.tv.shape[2], c.tv.shape[3], c.tv.device)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    ops = torch.ops.red_diffeq
    weff = (c.tE[None, :, :, None] * c.tW[:, None]).contiguous()
    v, w = c.tv.clone().requires_grad_(True), weff.clone().requires_grad_(True)
    opcheck(ops.enc_fwi, (v, w, plan.op_id, 1, True), test_utils=utils)
    opcheck(ops.enc_fwi, (c.tv, weff[:1].expand(c.B, -1, -1, -1), plan.op_id, 1, False), test_utils=utils)
    opcheck(ops.enc_fwi_ckpt, (v, w, plan.op_id, 1, 7), test_utils=utils)
    coeffs, vstat = ops.fwi_coeffs(c.tv, plan.op_id, 1)
    opcheck(ops.enc_fwi_forward, (coeffs, weff, plan.op_id, c.B, True), test_utils=utils)
    seis, hist = ops.enc_fwi_forward(coeffs, weff, plan.op_id, c.B, True)
    assert torch.equal(seis, c.reference()[0])
    for want in (True, False):
        opcheck(ops.enc_fwi_adjoint, (coeffs, weff, hist, c.tr, plan.op_id, c.B, want), test_utils=utils)
    gA, gk, gb, _ = ops.enc_fwi_adjoint(coeffs, weff, hist, c.tr, plan.op_id, c.B, False)
    opcheck(ops.enc_fwi_grad_finalize, (coeffs, vstat, gA, gk, gb, plan.op_id, c.B, c.ne, 1), test_utils=utils)
    opcheck(ops.enc_fwi_forward_ckpt, (coeffs, weff, plan.op_id, c.B, 7), test_utils=utils)
    _, ckpt = ops.enc_fwi_forward_ckpt(coeffs, weff, plan.op_id, c.B, 7)
    seg = torch.empty(int(plan.ckpt_sizes_enc(c.B, c.ne, 7).seg) // 4, device=cuda)
    opcheck(ops.enc_fwi_adjoint_ckpt, (coeffs, weff, ckpt, seg, c.tr, plan.op_id, c.B, 7, True), test_utils=utils)
    with pytest.raises(ValueError, match="expected fp32 effective wavelets"):
        ops.enc_fwi_forward(coeffs, weff[:, :, :1], plan.op_id, c.B, False)
    with pytest.raises(ValueError, match="do not match"):
        ops.enc_fwi_grad_finalize(coeffs, vstat, gA, gk, gb, plan.op_id, c.B, c.ne + 1, 1)
    fwi.check()


@pytest.mark.parametrize("ckpt", [None, 40])
def test_no_gradient_in_codes_or_wavelet_requests_no_gwav(cuda, cases, ckpt, monkeypatch):
    """Neither E nor the wavelet requires grad: the adjoint op is called with want_gw = False, gives the kernel no
    gwav and allocates none; v.grad is the same bits either way."""
    c = cases["tiles"]
    name = "enc_fwi_adjoint" if ckpt is None else "enc_fwi_adjoint_ckpt"
    seen = accumulators(monkeypatch, [name])
    fwi = c.fwi(checkpoint=ckpt)
    _, gv_only, _, _ = c.gradients(fwi, want=(True, False, False))
    _, gv, gW, gE = c.gradients(fwi)
    _, none, _, gE_only = c.gradients(fwi, want=(False, False, True))
    fwi.check()
    shapes = [tuple(out[3].shape) for out in seen[name]]
    assert shapes == [(0,), (c.B, c.ne, c.ns, c.nt), (c.B, c.ne, c.ns, c.nt)], shapes
    assert torch.equal(gv_only, gv) and torch.equal(gE_only, gE) and none is None


def test_fresh_code_tensors_are_read_afresh(cuda, cases):
    """A second call with another code tensor, and a second call with the SAME tensor changed in place, give those
    codes' result: no stale cached graph arguments, no stale copy."""
    c = cases["tiles"]
    fwi = c.fwi()
    with torch.no_grad():
        a = fwi(c.tv, wavelet=c.tW, encoding=c.tE)
        other = (c.tE.flip(1) * 0.5).contiguous()
        b = fwi(c.tv, wavelet=c.tW, encoding=other)
        assert torch.equal(a, c.reference()[0]) and not torch.equal(a, b)
        buf = c.tE.clone()
        assert torch.equal(fwi(c.tv, wavelet=c.tW, encoding=buf), a)
        buf.copy_(other)
        assert torch.equal(fwi(c.tv, wavelet=c.tW, encoding=buf), b)      # same tensor, new contents
        assert torch.equal(fwi(c.tv, wavelet=c.tW, encoding=c.tE), a)
        assert torch.equal(fwi(c.tv, wavelet=c.tW, encoding=c.tE[:2]), a[:, :2])     # another ne on the same plan
    fwi.check()


def test_default_wavelet_one_hot(cuda, cases):
    """wavelet=None uses the plan's (Ricker) signature: one-hot rows are the default call's records, bit for bit
    (whatever kernels the default call runs), and encode() with one-hot codes picks the same records."""
    from red_diffeq.utils.encoding import encode
    c = cases["tiles"]
    fwi = c.fwi()
    eye = torch.eye(c.ns, device=cuda)
    with torch.no_grad():
        shots = fwi(c.tv)
        enc = fwi(c.tv, encoding=eye)
    fwi.check()
    assert torch.equal(enc, shots) and torch.equal(encode(shots, eye), shots)
