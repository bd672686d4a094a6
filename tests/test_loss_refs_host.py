"""The references, case tables and inputs of tests/test_gpu_losses.py (tests/loss_refs.py), checked on the
CPU: the mixed references against the reference project's recorded TV / Tikhonov values, the full ones
against fp64 autograd of the formulas written out here, every case against the conditions the GPU tests
rely on, and the mixed references against the full ones inside the GPU tests' bars.  Nothing is skipped
or filtered: every case of the tables is checked."""
import numpy as np
import pytest
import torch

import loss_refs as R
from conftest import load_golden

U = R.U


# ------------------------------------------------------------------------------------------- tables
def test_tables_are_the_full_products():
    sizes = R.k5_sizes()
    four_d = [s for s, (shape, _) in sizes.items() if len(shape) == 4]
    assert len(sizes) == 12 and four_d == ["record"]
    assert len(R.k5_forward_cases()) == 12 * (len(R.K5_MASKS) - 1) + len(four_d)
    assert len(set(R.k5_forward_cases())) == len(R.k5_forward_cases())
    assert {s for s, _ in R.k5_backward_cases()} == {s for s, (shape, _) in sizes.items() if shape[0] == 3} | {"record"}
    assert len(R.k6_cases()) == (2 * len(R.K6_SHAPES) + 1) * len(R.K6_INPUTS)
    assert set(R.K6_WHY) == set(R.K6_SHAPES)


def test_k5_sizes_at_the_current_constants():
    """With L1_BLOCK = 256 and L1_ITEMS = 16 the table is the one the sizes were chosen as; with other
    constants the sizes move and only test_k5_size_hits_its_branches speaks."""
    blk, items, _, _ = R.kernel_constants()
    if (blk, items) != (256, 16):
        return
    shapes = [shape for shape, _ in R.k5_sizes().values()]
    assert shapes == [(3, n) for n in (1, 255, 256, 257, 4095, 4096, 4097, 8193)] + [
        (1, 5, 1000, 70), (2, 300 * 4096 + 5), (1, 1799 * 4096 + 1), (1, 2050 * 4096 + 77)]


@pytest.mark.parametrize("size", list(R.k5_sizes()))
def test_k5_size_hits_its_branches(size):
    """Each K5 size runs the branches it is in the table for, from the two kernel constants alone."""
    shape, want = R.k5_sizes()[size]
    got = R.k5_branches(int(np.prod(shape[1:])))
    assert got == want, (size, got, want)


def test_k5_branch_walk_on_known_counts():
    """k5_branches itself, at counts worked out by hand for L1_BLOCK = 256: 1800 chunks give threads
    0..7 one unrolled pass (chunks t .. t + 1792) and nothing after, threads 8..255 seven or fewer tail
    additions; 2051 chunks give every thread one unrolled pass and threads 0..2 chunk 2048 + t."""
    blk, items, _, _ = R.kernel_constants()
    if blk != 256:
        return
    b = R.k5_branches(1799 * blk * items + 1)
    assert (b["nchunk"], b["unrolled"], b["unrolled_then_tail"], b["tail_only"]) == (1800, 8, 0, 248)
    b = R.k5_branches(2050 * blk * items + 77)
    assert (b["nchunk"], b["unrolled"], b["unrolled_then_tail"], b["tail_only"]) == (2051, 256, 3, 0)
    b = R.k5_branches(256 * blk * items)
    assert (b["nchunk"], b["clamped"], b["strided"]) == (256, False, False)
    assert R.k5_branches(256 * blk * items + 1)["strided"]


@pytest.mark.parametrize("H,W", R.K6_SHAPES)
def test_k6_shape_classes_and_passes(H, W):
    """Every K6 shape has a cell of each class it can have, the spike cells sit in the classes they are
    named for and cover them, and the forward's pass count is the one the shape is listed for."""
    cls = R.cell_classes(H, W)
    assert cls.shape == (H, W)
    possible = R.classes_possible(H, W)
    assert sorted(set(cls.reshape(-1).tolist())) == possible
    assert (cls == 0).sum() == 4
    assert (cls == 1).sum() == 2 * (H - 2) + 2 * (W - 2) and (cls == 2).sum() == (H - 2) * (W - 2)
    # a cell's class is its number of neighbour terms: 2, 3, 4
    z, x = np.mgrid[:H, :W]
    terms = (x + 1 < W).astype(int) + (x > 0) + (z + 1 < H) + (z > 0)
    assert np.array_equal(terms, cls + 2)
    cells = R.spike_cells(H, W)
    assert len(set(cells.values())) == len(cells)
    for name, (cz, cx) in cells.items():
        want = 0 if name.startswith("corner") else 2 if name == "interior" else 1
        assert cls[cz, cx] == want, (name, cz, cx)
    assert sorted({int(cls[c]) for c in cells.values()}) == possible
    assert len(cells) == 4 + 2 * (W > 2) + 2 * (H > 2) + (H > 2 and W > 2)
    if R.kernel_constants()[2:] == (8, 256):
        assert R.k6_passes(H, W) == R.K6_WHY[(H, W)]["passes"]
    assert (H * W < 256, H * W == 256) == ((H, W) in ((2, 2), (2, 9), (9, 2)), (H, W) == (16, 16))


# ------------------------------------------------------------------------------------------- references
def test_mixed_smooth_reference_reproduces_the_recorded_losses():
    """tests/golden/small_losses.npz: the reference project's total_variation_loss / tikhonov_loss."""
    z = load_golden("small_losses")
    np.testing.assert_allclose(R.smooth_mixed(z["a"], R.TV), z["tv"], rtol=1e-6)
    np.testing.assert_allclose(R.smooth_mixed(z["a"], R.L2), z["l2"], rtol=1e-6)
    np.testing.assert_allclose(R.smooth_full(z["a"], R.TV)[0], z["tv"], rtol=1e-6)
    np.testing.assert_allclose(R.smooth_full(z["a"], R.L2)[0], z["l2"], rtol=1e-6)


@pytest.mark.parametrize("kind", R.K5_MASKS)
def test_full_l1_reference_is_autograd_of_the_formula(kind):
    """l1_full against the masked mean written model by model: sum |y - p| m / max(sum m, 1)."""
    shape = (3, 2, 50, 7)
    pred, y, mask = R.k5_inputs(shape, kind)
    gout = np.array(R.K5_GOUT)
    loss, nobs, grad = R.l1_full(pred, y, mask, gout)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    t = torch.from_numpy(y).double()
    m = torch.ones(shape, dtype=torch.float64) if mask is None else torch.from_numpy(mask).double()
    total = 0.0
    for b in range(3):
        cnt = max(float(m[b].sum()), 1.0)
        lb = ((t[b] - p[b]).abs() * m[b]).sum() / cnt
        np.testing.assert_allclose(loss[b], lb.item(), rtol=1e-13)
        assert nobs[b] == cnt
        total = total + gout[b] * lb
    total.backward()
    np.testing.assert_allclose(grad, p.grad.numpy(), rtol=1e-13, atol=0)
    # and in closed form: sign(p - y) m gout / nobs
    closed = np.sign(pred.astype(np.float64) - y) * m.numpy() * (gout / nobs).reshape(3, 1, 1, 1)
    np.testing.assert_allclose(grad, closed, rtol=1e-13, atol=0)


@pytest.mark.parametrize("kind", [R.TV, R.L2])
@pytest.mark.parametrize("H,W,inp", [(9, 2, "uniform"), (2, 9, "layered"), (16, 17, "uniform"), (16, 17, "layered"),
                                     (5, 6, "checker"), (4, 5, "spike")])
def test_full_smooth_reference_is_autograd_of_the_formula(H, W, inp, kind):
    """smooth_full against the two means written model by model, and smooth_terms against its gradient."""
    mu = R.k6_input(H, W, 3, inp, (H // 2, W // 2) if inp == "spike" else None)
    gout = R.k6_gout(3)
    loss, grad = R.smooth_full(mu, kind, gout)
    m = torch.from_numpy(mu).double().requires_grad_(True)
    f = torch.abs if kind == R.TV else torch.square
    total = 0.0
    for b in range(3):
        lx = sum(f(m[b, 0, zz, xx + 1] - m[b, 0, zz, xx]) for zz in range(H) for xx in range(W - 1)) / (H * (W - 1))
        ly = sum(f(m[b, 0, zz + 1, xx] - m[b, 0, zz, xx]) for zz in range(H - 1) for xx in range(W)) / ((H - 1) * W)
        np.testing.assert_allclose(loss[b], (lx + ly).item(), rtol=1e-12)
        total = total + float(gout[b]) * (lx + ly)
    total.backward()
    terms = R.smooth_terms(mu, kind, gout)
    M = np.abs(terms).sum(0)
    assert (np.abs(grad - m.grad.numpy()) <= 1e-13 * M).all()
    assert (np.abs(grad - terms.sum(0)) <= 1e-13 * M).all()
    assert np.array_equal(R.smooth_term_sum(mu, kind, gout), M)


@pytest.mark.parametrize("kind", [R.TV, R.L2])
def test_smooth_terms_are_the_gradient_at_the_large_shape(kind):
    mu = R.k6_input(502, 3002, 1, "uniform")
    gout = R.k6_gout(1)
    _, grad = R.smooth_full(mu, kind, gout)
    terms = R.smooth_terms(mu, kind, gout)
    M = np.abs(terms).sum(0)
    assert (np.abs(grad - terms.sum(0)) <= 1e-13 * M).all()
    assert np.array_equal(R.smooth_term_sum(mu, kind, gout), M)


# ------------------------------------------------------------------------------------------- K5 cases
@pytest.mark.parametrize("size,kind", R.k5_forward_cases())
def test_k5_case_conditions_and_mixed_within_bars(size, kind):
    """The inputs are what the table says, and the mixed K5 forward is within the GPU test's bar of the
    full one: 3 2^-24 relative (the subtraction, the product, the final cast), 4 with a fractional mask."""
    shape = R.k5_shape(size)
    pred, y, mask = R.k5_inputs(shape, kind)
    B, n = shape[0], int(np.prod(shape[1:]))
    assert pred.dtype == y.dtype == np.float32 and pred.shape == y.shape == shape
    loss, nobs = R.l1_mixed(pred, y, mask)
    loss64, nobs64, _ = R.l1_full(pred, y, mask)
    if kind == "none":
        assert mask is None and (nobs == n).all()
    else:
        assert mask.shape == shape and mask.dtype == (np.bool_ if kind == "bool" else np.float32)
        vals = set(np.unique(mask).tolist())
        assert vals <= ({0.0, 0.5, 1.0} if kind == "frac" else {0.0, 1.0})
        if n >= 255 and not (kind == "zero_model" and B == 1):    # B = 1: the only model is the all-zero one
            assert vals ==({0.0, 0.5, 1.0} if kind == "frac" else {0.0, 1.0})
        if kind in ("rand01", "bool", "eq") and n >= 255:
            assert 0.2 < 1 - mask.mean() < 0.4
    if kind == "zero_model":
        b0 = R.zero_model(B)
        assert mask[b0].astype(np.float64).sum() == 0.0                 # the all-zero model really sums to 0
        assert nobs[b0] == 1.0 and loss[b0] == 0.0 and loss64[b0] == 0.0  # nobs clamps to 1
        assert all(mask[b].any() for b in range(B) if b != b0 and n >= 255)
    if kind == "columns":
        col = mask[:, :1, :1, :]
        assert np.array_equal(mask, np.broadcast_to(col, shape))          # whole receivers, every shot and sample
        assert ((col == 0).sum(axis=3) >= 1).all() and ((col == 1).sum(axis=3) >= 1).all()
    same = pred.view(np.int32) == y.view(np.int32)
    if kind == "eq":
        assert same.any() and (n < 255 or 0.05 < same.mean() < 0.15)
    else:
        assert not same.any()
    assert np.array_equal(nobs.astype(np.float64), nobs64) or kind == "frac"
    assert (np.abs(nobs - nobs64) <= U * nobs64).all()
    bar = (4 if kind == "frac" else 3) * U * loss64
    assert (np.abs(loss.astype(np.float64) - loss64) <= bar).all(), (size, kind, loss, loss64)


@pytest.mark.parametrize("size,kind", R.k5_backward_cases())
def test_k5_backward_mixed_within_bar(size, kind):
    """The mixed backward is within 2 2^-24 relative of fp64 autograd (the division, the product), and
    exactly 0 where pred == y or the mask is 0."""
    shape = R.k5_backward_shape(size)
    pred, y, mask = R.k5_inputs(shape, kind)
    gout = np.array(R.K5_GOUT, np.float32)
    _, nobs = R.l1_mixed(pred, y, mask)
    got = R.l1_backward_mixed(pred, y, mask, nobs, gout)
    _, _, ref = R.l1_full(pred, y, mask, gout)
    assert got.shape == ref.shape == shape
    assert (np.abs(got - ref) <= 2 * U * np.abs(ref)).all()
    zero = pred == y
    if mask is not None:
        zero |= mask == 0
    assert (got[zero] == 0).all() and (ref[zero] == 0).all()
    assert (got[1] == 0).all()                                          # gout = 0
    nz = ~zero
    nz[1] = False
    assert (got[nz] != 0).all()


# ------------------------------------------------------------------------------------------- K6 cases
@pytest.mark.parametrize("H,W,B,inp", R.k6_cases())
def test_k6_case_conditions_and_mixed_within_bars(H, W, B, inp):
    """The inputs meet the conditions the GPU tests rely on, and the mixed K6 forward is within the GPU
    test's bars of the full one: TV 4 2^-24 relative, Tikhonov 5 2^-24 (all terms are non-negative)."""
    n = 0
    for label, mu in R.k6_variants(H, W, B, inp):
        n += 1
        assert mu.shape == (B, 1, H, W) and mu.dtype == np.float32
        assert not R.bad_differences(mu).any()        # every difference is exactly 0 or at least MIN_DIFF
        m64 = mu.astype(np.float64)
        dx, dy = np.diff(m64, axis=3), np.diff(m64, axis=2)
        if inp == "layered":
            assert (dx == 0).mean() >= 0.3 and (dy == 0).mean() >= 0.3
            assert B == 1 or not np.array_equal(mu[0], mu[1])
            assert (dx != 0).any() and (dy != 0).any()
        if inp == "uniform":
            assert (dx != 0).all() and (dy != 0).all()
        if inp == "constant":
            assert not dx.any() and not dy.any()
        if inp == "checker":
            assert (np.abs(dx) == 2).all() and (np.abs(dy) == 2).all()
        if inp == "spike":
            cz, cx = R.spike_cells(H, W)[label]
            flat = mu.copy()
            assert (flat[:, 0, cz, cx] != 0.25).all()
            flat[:, 0, cz, cx] = 0.25
            assert (flat == 0.25).all()
        for kind, k in ((R.TV, 4), (R.L2, 5)):
            got = R.smooth_mixed(mu, kind).astype(np.float64)
            ref, _ = R.smooth_full(mu, kind)
            assert (np.abs(got - ref) <= k * U * ref).all(), (label, kind, got, ref)
            if inp == "constant":
                assert not got.any() and not ref.any()
    assert n == (len(R.spike_cells(H, W)) if inp == "spike" else 1)
