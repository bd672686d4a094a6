"""The K13 test module's own parts on the CPU (tests/misfit_refs.py): the two references of every kind against
each other, the branch each size of the tables is for (from the kernels' constants, read out of
csrc/misfit.hip), the host-only C entry points, and the Python entry points' signatures and argument checks.

Bars between the two references (u = 2^-24, e = 2^-53; misfit_refs.bar(k) compounds k fp32 roundings):
L2 / Huber forward   mixed rounds d to fp32 (d d then carries 2 u; Huber's rho likewise: rho' <= d / delta, so
                     an error u |d| in d is at most 2 u rho in the quadratic zone and 2 u rho in the tails, where
                     rho >= |d| / 2) and the loss once; every term is non-negative, so the per-term bound carries
                     to the sum: bar(3), bar(4) with a fractional mask (nobs is then rounded to fp32 too).
L2 / Huber backward  d (1) and the final rounding (1): bar(2) relative; exactly 0 where mask == 0 or d == 0.
NCC                  the products are exact in fp64, so the references differ by fp64 roundings only.  With
                     eps = 2 nt e bounding two summation orders of nt terms relative to the sum of their absolute
                     values (Q <= sqrt(a c) for q, by Cauchy-Schwarz), the cosine moves by at most 2 eps + 4 e and
                     J = 1 - cos by 2 e more: |dJ| <= 2 eps + 8 e.  loss: u |loss| + 2 (2 eps + 8 e).  Gradient:
                     the final rounding (1) plus the fp64 stages, far below u for nt < 2^20: 2 u M, M the sum of
                     the absolute values of the element's two terms."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import misfit_refs as R

U, E = R.U, R.E


def ncc_j_bar(nt):
    return 2 * (2 * nt * E) + 8 * E


# ------------------------------------------------------------------------------ references agree
@pytest.mark.parametrize("kind", ["l2", "huber"])
@pytest.mark.parametrize("size,mask_kind", [(s, m) for s, m in R.mf_forward_cases() if s != "strided"])
def test_mf_mixed_and_full_agree(kind, size, mask_kind):
    shape = R.mf_backward_shape(size)
    pred, y, mask = R.mf_inputs(kind, shape, mask_kind)
    loss, nobs = R.mf_mixed(kind, pred, y, mask)
    gout = np.array(R.GOUT, np.float32)
    full, full_nobs, grad = R.mf_full(kind, pred, y, mask, gout)
    k = 4 if mask_kind == "frac" else 3
    assert (np.abs(nobs - full_nobs) <= U * full_nobs).all()
    assert (np.abs(loss.astype(np.float64) - full) <= R.bar(k) * full).all(), (loss, full)
    got = R.mf_backward_mixed(kind, pred, y, mask, nobs, gout)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - grad) <= R.bar(2 + (mask_kind == "frac")) * np.abs(grad)).all()
    zero = pred == y
    if mask is not None:
        zero |= mask == 0
    assert (got[zero] == 0).all() and (grad[zero] == 0).all()
    if mask_kind == "zero_model":
        b0 = R.zero_model(shape[0])
        assert nobs[b0] == 1 and loss[b0] == 0 and not got[b0].any()


def test_huber_inputs_hold_every_special_element():
    """d is exact everywhere; |d| == delta, one ulp above and below it on both signs, and d == 0 all occur, at
    n = 1 too (one special per model), and the branch taken on them is the one the name says."""
    d = np.float32(R.DELTA)
    for size in ("n=1", "n=257", "record"):
        shape = R.mf_backward_shape(size)
        pred, y = R.mf_pair("huber", shape)
        diff = pred - y
        sp = R.huber_special(shape)
        want = {0: d, 1: -d, 2: np.nextafter(d, np.float32(1)), 3: np.nextafter(d, np.float32(0)),
                4: -np.nextafter(d, np.float32(1)), 5: -np.nextafter(d, np.float32(0)), 6: np.float32(0)}
        seen = set()
        for k, v in want.items():
            if (sp == k).any():
                assert (diff[sp == k] == v).all(), (size, k)
                seen.add(k)
        assert seen == ({1, 3, 5} if size == "n=1" else set(want)), (size, seen)
        quad = np.abs(diff) <= d
        assert quad[np.isin(sp, (0, 1, 3, 5, 6))].all() and not quad[np.isin(sp, (2, 4))].any()
    # rho and psi are continuous across the branch: one ulp either side of delta moves them by about an ulp
    a = R._rho("huber", np.array([want[3], want[0], want[2]], np.float32), R.DELTA)
    assert a[0] < a[1] < a[2] and a[2] - a[0] <= 4 * U * R.DELTA
    p = R._psi("huber", np.array([want[3], want[0], want[2]], np.float32), R.DELTA)
    assert p[0] < 1.0 and p[1] == 1.0 and p[2] == 1.0


@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("shape", [(3, 2, 37, 7), (3, 1, 129, 3), (3, 2, 1, 70)])
def test_ncc_mixed_and_full_agree(shape, mask_kind):
    pred, y, mask = R.ncc_inputs(shape, mask_kind)
    mx = R.ncc_mixed(pred, y, mask)
    gout = np.array(R.GOUT, np.float32)
    fl = R.ncc_full(pred, y, mask, gout)
    assert np.array_equal(mx["live"], fl["live"]) and np.array_equal(mx["ntr"].astype(np.float64), fl["ntr"])
    assert np.isfinite(fl["grad"]).all()
    assert (np.abs(mx["J"] - fl["J"]) <= ncc_j_bar(shape[2])).all()
    assert (np.abs(mx["loss"].astype(np.float64) - fl["loss"]) <= U * np.abs(fl["loss"]) + 2 * ncc_j_bar(shape[2])).all()
    got, M = R.ncc_backward_mixed(pred, y, mask, mx["inv"], mx["r"], mx["ntr"], gout)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - fl["grad"]) <= 2 * U * M).all()
    dead = np.broadcast_to((~mx["live"])[:, :, None, :], shape)
    assert (got[dead] == 0).all() and (fl["grad"][dead] == 0).all()
    if mask_kind == "zero_model":
        b0 = R.zero_model(3)
        assert mx["ntr"][b0] == 1 and mx["loss"][b0] == 0


def test_ncc_formula_properties_in_fp64():
    """The exact cases on the CPU: dead traces and zero predicted traces (J, gradient, ntr), orthogonality of
    the gradient to the predicted trace, pred == y, and pred -> 2^k pred."""
    pred, y, mask, dead, zero_pred = R.ncc_exact_case()
    gout = np.array(R.GOUT, np.float32)
    mx = R.ncc_mixed(pred, y, mask)
    fl = R.ncc_full(pred, y, mask, gout)
    assert np.array_equal(~mx["live"], dead) and (mx["J"][dead] == 0).all() and (mx["J"][zero_pred] == 1).all()
    assert mx["ntr"].tolist() == [(~dead[0]).sum(), 1.0, (~dead[2]).sum()] and mx["loss"][1] == 0
    got, M = R.ncc_backward_mixed(pred, y, mask, mx["inv"], mx["r"], mx["ntr"], gout)
    off = np.broadcast_to((dead | zero_pred)[:, :, None, :], pred.shape)
    assert (got[off] == 0).all() and (fl["grad"][off] == 0).all()
    assert (np.abs(got.astype(np.float64) - fl["grad"]) <= 2 * U * M).all()
    orth = np.abs((got.astype(np.float64) * pred).sum(2))
    assert (orth <= (2 * U * M * np.abs(pred)).sum(2)).all()
    same = R.ncc_mixed(y, y, mask)
    g_same, _ = R.ncc_backward_mixed(y, y, mask, same["inv"], same["r"], same["ntr"], gout)
    assert not g_same.any() and (np.abs(same["J"]) <= 4 * E).all()
    for k in (-3, 5):
        sc = R.ncc_mixed(pred * np.float32(2.0 ** k), y, mask)
        assert np.array_equal(sc["J"], mx["J"]) and np.array_equal(sc["loss"], mx["loss"])
        g_sc, _ = R.ncc_backward_mixed(pred * np.float32(2.0 ** k), y, mask, sc["inv"], sc["r"], sc["ntr"], gout)
        assert np.array_equal(g_sc * np.float32(2.0 ** k), got)


# ------------------------------------------------------------------------------ the tables hit their branches
def test_mf_sizes_hit_their_branches():
    c = R.kernel_constants()
    assert c["MF_BLOCK"] >= 2 and c["MF_ITEMS"] >= 2
    for name, (shape, want) in R.mf_sizes().items():
        n = int(np.prod(shape[1:]))
        assert R.mf_branches(n) == want, (name, R.mf_branches(n), want)
    assert any(w["strided"] for _, w in R.mf_sizes().values())


def test_ncc_shapes_hit_their_branches():
    c = R.kernel_constants()
    tc, blk, un = c["NCC_TC"], c["NCC_BLOCK"], c["NCC_UNROLL"]
    for nt, (why, ntc) in R.ncc_nt().items():
        for ng, want in R.ncc_ng().items():
            br = R.ncc_branches(nt, ng)
            assert br["ntc"] == ntc and br["tiles"] == want["tiles"] and br["ctiles"] == len(want["tiles"]), (nt, ng, br)
    assert R.ncc_branches(tc, 1)["idle"] == blk - tc               # more phases than rows
    assert R.ncc_branches(1, 70)["idle"] == 140 and R.ncc_branches(1, 70)["tail"] == 70
    assert R.ncc_branches(tc, 70)["unrolled"] == 210 and R.ncc_branches(tc, 70)["tail"] == 210   # 21 or 22 rows a thread
    assert tc % (un * 4) == 0 and R.ncc_branches(tc, 64)["tail"] == 0   # 16 rows a thread: the unrolled loop alone
    assert R.ncc_branches(tc + 1, 64)["tail"] == 64                # the second chunk's single row
    rec = R.ncc_branches(R.RECORD[2], R.RECORD[3])
    assert rec["ntc"] == -(-1000 // tc) and rec["tiles"] == [(70, 3, 210)]
    shapes = R.ncc_shapes()
    assert len(shapes) == 2 * 5 * 6 + 1 and R.RECORD in shapes


# ------------------------------------------------------------------------------ host-only C entry points
def test_workspace_and_coef_bytes_without_a_gpu():
    from red_diffeq import _hip
    from red_diffeq.ops import MISFIT_KINDS
    L = _hip.load_library()
    c = R.kernel_constants()
    chunk, tc, blk = c["MF_BLOCK"] * c["MF_ITEMS"], c["NCC_TC"], c["NCC_BLOCK"]
    assert MISFIT_KINDS == {"l2": 1, "huber": 2, "ncc": 3}
    for B, ns, nt, ng in ((2, 5, 1000, 70), (3, 1, 1, 1), (1, 16, 1000, 3000), (3, 2, tc + 1, blk + 1)):
        n = ns * nt * ng
        for kind in (1, 2):
            assert L.rdq_misfit_workspace_bytes(kind, B, ns, nt, ng) == B * -(-n // chunk) * 2 * 8
            assert L.rdq_misfit_coef_bytes(kind, B, ns, ng) == 0
        want = (B * ns * -(-nt // tc) * 3 * ng + B * -(-ns * ng // blk) * 2) * 8
        assert L.rdq_misfit_workspace_bytes(3, B, ns, nt, ng) == want
        assert L.rdq_misfit_coef_bytes(3, B, ns, ng) == B * ns * ng * 3 * 8
    for bad in ((0, 1, 1, 1, 1), (4, 1, 1, 1, 1), (1, 0, 1, 1, 1), (3, 1, 0, 1, 1), (3, 1, 1, 0, 1), (2, 1, 1, 1, -1)):
        assert L.rdq_misfit_workspace_bytes(*bad) == 0
    # argument checks come before any launch: no GPU is touched
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)            # a non-null placeholder, never dereferenced: the call is refused first
    for kind, dims, delta in ((0, (1, 1, 1, 1), 0.0), (4, (1, 1, 1, 1), 0.0), (1, (0, 1, 1, 1), 0.0),
                              (1, (1, 1, 1, -2), 0.0), (2, (1, 1, 1, 1), 0.0), (2, (1, 1, 1, 1), -1.0),
                              (2, (1, 1, 1, 1), float("inf")), (2, (1, 1, 1, 1), float("nan"))):
        assert L.rdq_misfit_forward(kind, *dims, delta, one, one, null, one, one, one, one, st) == -10001
        assert L.rdq_misfit_backward(kind, *dims, delta, one, one, null, one, one, one, one, st) == -10001


# ------------------------------------------------------------------------------ Python entry points
def test_python_entry_points_keep_their_signatures():
    from red_diffeq.core import losses
    from red_diffeq.core.inversion import InversionEngine
    assert losses.MISFITS == ("l1", "l2", "huber", "ncc")
    assert list(inspect.signature(losses.misfit).parameters) == ["predicted", "target", "mask", "kind", "delta", "norm"]
    assert list(inspect.signature(losses.l1_misfit).parameters) == ["predicted", "target", "mask", "nobs"]
    p = inspect.signature(losses.LossCalculator.__init__).parameters
    assert list(p) == ["self", "regularization_method", "misfit", "huber_delta"]
    assert p["misfit"].default == "l1" and p["huber_delta"].default is None
    p = inspect.signature(InversionEngine.optimize).parameters
    assert list(p) == ["self", "mu", "mu_true", "y", "fwi_forward", "ts", "lr", "reg_lambda", "noise_std", "noise_type",
                       "missing_number", "regularization", "process_group", "misfit", "huber_delta"]
    assert p["misfit"].default == "l1" and p["huber_delta"].default is None
    import red_diffeq.ops  # noqa: F401
    ns = torch.ops.red_diffeq
    assert str(ns.misfit.default._schema) == ("red_diffeq::misfit(Tensor pred, Tensor y, Tensor? mask, SymInt kind, "
                                              "float delta) -> (Tensor, Tensor, Tensor)")
    assert str(ns.misfit_backward.default._schema) == (
        "red_diffeq::misfit_backward(Tensor pred, Tensor y, Tensor? mask, Tensor norm, Tensor coef, Tensor gout, "
        "SymInt kind, float delta) -> Tensor")


@pytest.mark.parametrize("kind,delta", [("l3", None), ("", None), (None, None), ("huber", None), ("huber", 0.0),
                                        ("huber", -0.5), ("huber", float("inf")), ("huber", float("nan")),
                                        ("huber", "x")])
def test_bad_misfit_arguments_raise_before_any_gpu_work(kind, delta):
    """An unknown kind, or huber without a finite delta > 0: ValueError from LossCalculator, misfit() and
    optimize(), on CPU tensors (the kernels would raise RuntimeError for those: the check comes first)."""
    from red_diffeq.core.inversion import InversionEngine
    from red_diffeq.core.losses import LossCalculator, misfit
    from red_diffeq.regularization.base import RegularizationMethod

    class dm:
        device = torch.device("cpu")

    with pytest.raises(ValueError, match="misfit|huber"):
        LossCalculator(RegularizationMethod(None), kind, delta)
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="misfit|huber"):
        misfit(x, x, None, kind, delta)
    eng = InversionEngine(dm, None, None, show_progress=False)
    with pytest.raises(ValueError, match="misfit|huber"):
        eng.optimize(torch.zeros(1, 1, 6, 6), torch.zeros(1, 1, 4, 4), x, lambda v: v, ts=1, misfit=kind,
                     huber_delta=delta)


def test_good_misfit_arguments_pass_the_check():
    from red_diffeq.core.losses import LossCalculator, check_misfit
    from red_diffeq.regularization.base import RegularizationMethod
    assert [check_misfit(k) for k in ("l1", "l2", "ncc")] == [0.0, 0.0, 0.0]
    assert check_misfit("huber", 0.25) == 0.25 and check_misfit("l2", -1.0) == 0.0
    c = LossCalculator(RegularizationMethod("tv"))
    assert c.misfit == "l1" and c.huber_delta is None and c.global_nobs is None
    c = LossCalculator(RegularizationMethod("tv"), "huber", 0.5)
    assert (c.misfit, c.huber_delta) == ("huber", 0.5)


def test_global_norm_is_the_kernels_predicate():
    """The sharded survey's normaliser from the replicated record: nobs for l2 / huber (K5's), and for ncc the
    number of traces with a non-zero masked observed sample, which is the mixed reference's live count."""
    from red_diffeq.core.losses import global_norm
    pred, y, mask, dead, _ = R.ncc_exact_case()
    mx = R.ncc_mixed(pred, y, mask)
    got = global_norm("ncc", torch.from_numpy(y), torch.from_numpy(mask))
    assert got.dtype == torch.float32 and got.tolist() == mx["ntr"].tolist()
    assert global_norm("ncc", torch.from_numpy(y), None).tolist() == R.ncc_mixed(pred, y, None)["ntr"].tolist()
    for kind in ("l1", "l2", "huber"):
        assert global_norm(kind, torch.from_numpy(y), torch.from_numpy(mask)).tolist() == R.mf_mixed("l2", pred, y, mask)[1].tolist()
        assert global_norm(kind, torch.from_numpy(y), None).tolist() == [float(y[0].size)] * 3
