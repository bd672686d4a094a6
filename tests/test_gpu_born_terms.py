"""The Born pass (k_dmax, k_dcoeffs, k_born_tb, Pass::born) per trace, per term and per prologue element against
fp64, where tests/test_gpu_born.py reduces a model's whole record to one number.

Fixtures: tests/golden/born.npz (dense directions) and tests/golden/born_terms.npz (single-cell directions that
isolate the tangent's four sources: dA in the model, dA replicated into the pad, dK in the sponge, dbeta at the
source cells; tests/golden/make_born.py).  The per-trace yardstick is tests/born_traces.py, made from the fixtures
alone; the prologue's expected values are the header's formulas (include/red_diffeq_fwi.h) in fp64 on the fp32
inputs.  Everything that is a property of the schedule, of linearity or of the buffers' state is bitwise."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import born_traces as T
from conftest import load_golden, record_margin
from test_gpu_born import Case, dot, identity_bound, rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # fp32 unit roundoff


class TermsCase(Case):
    """One direction of born_terms.npz with the attributes of test_gpu_born.Case."""

    def __init__(self, name, cuda):
        z = load_golden("born_terms")
        pre = "terms_ctx_"
        self.ctx = {k[len(pre):]: (z[k].item() if z[k].ndim == 0 else z[k].tolist()) for k in z.files
                    if k.startswith(pre)}
        self.tag, self.normalize, self.st = f"terms/{name}", bool(z["terms_normalize"]), int(z["terms_st"])
        self.v = torch.from_numpy(z["terms_v"]).to(cuda)
        self.w = torch.from_numpy(z["terms_w"]).to(cuda)
        self.jtw64 = torch.from_numpy(z["terms_jtw64"]).to(cuda)
        self.dv = torch.from_numpy(z[f"terms_{name}_dv"]).to(cuda)
        self.jdv64 = torch.from_numpy(z[f"terms_{name}_jdv64"]).to(cuda)
        self.eref = z[f"terms_{name}_eref"]
        self.ip = float(z[f"terms_{name}_ip"][0])


@pytest.fixture(scope="module")
def cases(cuda):
    out = {tag: Case(tag, cuda) for tag in T.DENSE}
    out.update({f"terms/{d}": TermsCase(d, cuda) for d in T.DIRECTIONS})
    return out


def randn(shape, seed, cuda):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(cuda)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """torch.equal on the bit patterns: a NaN equals itself, +0 differs from -0."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ per trace, per term
@pytest.mark.parametrize("case", T.ALL)
def test_born_per_trace_against_fp64(cuda, cases, case):
    """Every trace (b, s, g) of the record, the weak ones included (in `tiles` 45 % of the traces carry less than
    1e-3 of the strongest one's norm, which the per-model rel-L2 cannot see):
        ||ds - jdv64||  <=  4 max(e_ref, E_ref[b]) max(n64, 1e-12 N_b)
    with n64 = ||jdv64|| and e_ref = ||jdv32 - jdv64|| / n64 on that trace, N_b the model's largest n64.  The
    yardstick is the reference's own fp32 jvp error on the same trace (up to 7.6 E_ref, terms/argmin), never the
    HIP record; 4 is the project's factor for another valid fp32 operation order (tests/test_gpu_born.py).

    The floor.  The prologue scales a direction to max |dvs| in [2^-64, 2^-63), so a unit response (|J dv| =
    |dv|) sits 85 binades above the smallest denormal 2^-149; fp32 resolves 24 of them, so values down to 2^-61
    (4e-19) of a unit response keep full precision in the loop.  The fixtures' max |J dv| / max |dv| is 0.0048 ..
    0.0062 (wrap), 3.3 .. 4.2 (tiles), 2.7 (geom) and 0.008 .. 6.1 (terms), each model's record taken by itself (a
    terms direction over both of its models: 0.116 .. 6.1): at least 2^-8.  A trace at 1e-12 N_b (2^-40 of the
    strongest trace, whose norm over nrec = 160 samples is at most 2^4 times the record's peak) has samples around
    2^-40 2^-8 2^-4 = 2^-52 of a unit response: inside the resolved range with 9 binades to spare.
    Below the floor the bar is absolute, 4 max(e_ref, E_ref) 1e-12 N_b; no trace is left out."""
    c = cases[case]
    jdv64, jdv32, eref = T.records(case)
    ds = c.fwi().born(c.v, c.dv).cpu().numpy()
    assert np.isfinite(ds).all()
    ratio = T.trace_ratio(ds, jdv64, jdv32, eref)
    n64 = T.trace_norm(jdv64)
    rel = n64 / n64.reshape(n64.shape[0], -1).max(axis=1)[:, None, None]
    b, s, g = np.unravel_index(np.argmax(ratio), ratio.shape)
    weak = rel < 1e-3
    print(f"born per trace {case}: worst ratio to the factor-1 bar {ratio.max():.3f} at trace ({b}, {s}, {g}) "
          f"(n64 / N_b {rel[b, s, g]:.2e}); on the {int(weak.sum())} traces under 1e-3 N_b "
          f"{ratio[weak].max() if weak.any() else 0:.3f}; under the floor {int((rel < T.FLOOR).sum())}")
    record_margin("born_per_trace_over_bar", case, ratio.max(), 4.0)
    if weak.any():
        record_margin("born_per_trace_weak_over_bar", case, ratio[weak].max(), 4.0)
    assert (ratio <= 4).all(), (case, (b, s, g), float(ratio.max()))


@pytest.mark.parametrize("name", T.DIRECTIONS)
def test_born_per_term(cuda, cases, name):
    """One source of the tangent at a time (a single non-zero cell of dv per model): the per-model bar, and
    <born(v, dv), w> against sum(dv J^T w) in fp64 under the adjoint identity's bound."""
    c = cases[f"terms/{name}"]
    fwi = c.fwi()
    ds = fwi.born(c.v, c.dv)
    fwi.check()
    assert ds.shape == c.jdv64.shape
    err = rel_l2(ds, c.jdv64)
    for b, (e, eref) in enumerate(zip(err, c.eref)):
        print(f"born term {name}[{b}]: rel-L2 {e:.3e}, E_ref {eref:.3e}, ratio to the bar {e / (4 * eref):.3f}")
        record_margin("born_term_vs_fp64_over_4Eref", f"{name}[{b}]", e, 4 * eref)
    assert (err <= 4 * c.eref).all(), (name, err, c.eref)
    lhs, rhs = dot(ds, c.w), dot(c.dv, c.jtw64)
    bound = identity_bound(c, c.jdv64, c.w, c.dv, c.jtw64)
    print(f"born term {name}: <J dv, w> {lhs:.9e}, fp64 <dv, J^T w> {rhs:.9e}, bound {bound:.3e}")
    record_margin("born_term_scalar_over_bound", name, abs(lhs - rhs), bound)
    assert abs(rhs - c.ip) <= 1e-10 * abs(c.ip)
    assert abs(lhs - rhs) <= bound, (name, lhs, rhs, bound)


# ------------------------------------------------------------------------------------------ the prologue
class Prologue:
    """rdq_fwi_born_sizes + rdq_fwi_dcoeffs through plan.lib, as ops.fwi_born calls them, and the workspace read
    back with the layout the header gives: dam [B][nz][nx], ratio [B], dbeta [B][ns], oscale [B], uint32 dmax [B]."""

    def __init__(self, c, v, vel_mode):
        from red_diffeq import _hip
        from red_diffeq.solvers.pde import adj_sr
        self.hip = _hip
        self.fwi = c.fwi()
        self.B, _, self.nz, self.nx = v.shape
        self.plan = self.fwi._plan(self.nz, self.nx, v.device)
        self.vel_mode, self.v = vel_mode, v
        self.coeffs, self.vstat = self.plan.coeffs(v, vel_mode)
        x = self.fwi.ctx
        isx, isz = adj_sr(np.asarray(x["sx"]), x["sz"], np.asarray(x["gx"]), x["gz"], x["dx"], x["nbc"])[:2]
        self.src = [(min(max(int(isz) - x["nbc"], 0), self.nz - 1), min(max(int(i) - x["nbc"], 0), self.nx - 1))
                    for i in isx]
        self.ns = len(self.src)
        nbytes = ctypes.c_size_t()
        _hip.check(self.plan.lib.rdq_fwi_born_sizes(self.plan.handle, self.B, ctypes.byref(nbytes)), "born_sizes")
        self.n = self.B * self.nz * self.nx
        assert nbytes.value == 4 * (self.n + 3 * self.B + self.B * self.ns + 4)
        self.words = nbytes.value // 4

    def new_work(self, fill=0.0):
        return torch.full((self.words,), fill, dtype=torch.float32, device=self.v.device)

    def run(self, dv, dwork=None):
        """The workspace after one prologue on direction `dv` (any view), as int32 words on the device."""
        if dwork is None:
            dwork = self.new_work()
        P = self.hip.ptr
        assert dv.dtype == torch.float32 and tuple(dv.shape) == (self.B, 1, self.nz, self.nx)
        strides = (ctypes.c_int64 * 4)(*dv.stride())
        self.hip.check(self.plan.lib.rdq_fwi_dcoeffs(self.plan.handle, self.B, P(dv), strides, self.vel_mode,
                                                     P(self.coeffs), P(self.vstat), P(dwork),
                                                     self.hip.stream_of(self.coeffs)), "rdq_fwi_dcoeffs")
        torch.cuda.synchronize()
        return dwork.view(torch.int32)[:self.words - 4].clone()              # the four spare words are not written

    def split(self, words):
        w = words.cpu().numpy()
        B, n, ns = self.B, self.n, self.ns
        f = w.view(np.float32)
        return {"dam": f[:n].reshape(B, self.nz, self.nx), "ratio": f[n:n + B],
                "dbeta": f[n + B:n + B + B * ns].reshape(B, ns), "oscale": f[n + B + B * ns:n + 2 * B + B * ns],
                "dmax": w[n + 2 * B + B * ns:n + 3 * B + B * ns].view(np.uint32)}

    def expected(self, dv):
        """The header's formulas in fp64 on the fp32 inputs (v, dv, and dt, dx as the plan holds them)."""
        x = self.fwi.ctx
        dt, dx = float(np.float32(x["dt"])), float(np.float32(x["dx"]))
        v = self.v.cpu().numpy().astype(np.float64)[:, 0]
        d32 = dv.cpu().numpy()[:, 0]
        if self.vel_mode == 0:
            v = (v + 1) / 2 * 3000 + 1500
        amax = np.abs(d32).reshape(self.B, -1).max(axis=1)
        # k = floor(log2 max |dv|) + 64 within [-63, 126] (a zero direction: -63); 2^k = oscale
        k = np.clip(np.where(amax > 0, np.frexp(amax.astype(np.float64))[1] - 1 + 64, -63), -63, 126)
        dvs = d32.astype(np.float64) * (2.0 ** -k.astype(np.float64))[:, None, None]
        top = np.abs(dvs).reshape(self.B, -1).max(axis=1)
        assert (((top >= 2.0 ** -64) | (k == -63)) & ((top < 2.0 ** -63) | (k == 126))).all()
        if self.vel_mode == 0:
            dvs = dvs * 1500
        out = {"dmax": amax.view(np.uint32), "oscale": 2.0 ** k.astype(np.float64),
               "dam": 2 * (v * dt / dx) * (dvs * dt / dx)}
        flat = v.reshape(self.B, -1)
        am = flat.argmin(axis=1)                              # first row-major minimum
        out["ratio"] = dvs.reshape(self.B, -1)[np.arange(self.B), am] / flat[np.arange(self.B), am]
        out["dbeta"] = np.array([[2 * (v[b, iz, ix] * dt) * (dvs[b, iz, ix] * dt) for iz, ix in self.src]
                                 for b in range(self.B)])
        return out, am


# fp32 roundings on each value's path, counted in k_coeffs / k_vstat_* (the model copy and vmin: v + 1, x 3000, + 1500;
# the / 2 is exact) and k_dcoeffs (the power-of-two scale and the 2 x are exact):
#   dam    model copy 3, x dt, / dx | dv: x 1500, x dt, / dx | the product          3 + 2 + 3 + 1 = 9  (physical: 5)
#   ratio  vmin 3 | dv: x 1500 | the quotient                                       3 + 1 + 1     = 5  (physical: 1)
#   dbeta  model copy 3, x dt | dv: x 1500, x dt | the product                      3 + 1 + 2 + 1 = 7  (physical: 3)
# dt and dx enter as the fp32 values the plan holds, on both sides.
ROUNDINGS = {0: {"dam": 9, "ratio": 5, "dbeta": 7}, 1: {"dam": 5, "ratio": 1, "dbeta": 3}}
MAGNITUDES = (2.0 ** -100, 1.0, 2.0 ** 90)


def check_workspace(p, dv, label):
    """One prologue on `dv` against Prologue.expected: dmax and oscale exactly, dam / ratio / dbeta per element within
    their roundings x 2^-24, an exact zero where the fp64 value is zero.  Returns the number of zeros per field."""
    got, (want, am) = p.split(p.run(dv)), p.expected(dv)
    vstat = p.vstat.cpu().numpy()
    off = (4 * p.B + 15) // 16 * 16                                    # vstat: float vmin [B], then int64 argmin [B]
    assert (vstat[off:off + 8 * p.B].view(np.int64) == am).all()       # K3's argmin is the fp64 one
    assert (got["dmax"] == want["dmax"]).all(), (got["dmax"], want["dmax"])
    assert (got["oscale"].astype(np.float64) == want["oscale"]).all(), (got["oscale"], want["oscale"])
    zeros = {}
    for name, k in ROUNDINGS[p.vel_mode].items():
        g, w = got[name].astype(np.float64), want[name]
        assert np.isfinite(g).all() and g.shape == w.shape
        zero = w == 0
        assert (g[zero] == 0).all(), name
        zeros[name] = int(zero.sum())
        err = np.abs(g - w)[~zero] / np.abs(w[~zero])
        print(f"prologue {label} {name}: worst relative error {err.max() / U:.2f} x 2^-24, bar {k} x 2^-24")
        record_margin(f"born_prologue_{name}_over_roundings", label, err.max(), k * U)
        assert (err <= k * U).all(), (name, float(err.max() / U), k)
    return zeros


def prologue_inputs(cases, model, vel_mode, cuda):
    """B = 3 copies of the model's first member in the units of vel_mode, and a dense randn direction per model
    with magnitudes 2^-100, 1, 2^90 and an exact zero in each: at an ordinary cell, at the argmin, under shot 0."""
    c = cases[model]
    v = c.v[:1]
    if c.normalize and vel_mode == 1:
        v = (v + 1) / 2 * 3000 + 1500
    if not c.normalize and vel_mode == 0:
        v = (v - 1500) / 3000 * 2 - 1
    v = v.repeat(3, 1, 1, 1).contiguous()
    p = Prologue(c, v, vel_mode)
    dv = randn(v.shape, 61, cuda) * (0.04 if vel_mode == 0 else 60.0)
    dv = dv * torch.tensor(MAGNITUDES, dtype=torch.float32, device=cuda)[:, None, None, None]
    am = int(p.expected(dv)[1][1])
    dv[0, 0, 3, 4] = 0.0
    dv[1, 0, am // p.nx, am % p.nx] = 0.0
    dv[2, 0, p.src[0][0], p.src[0][1]] = 0.0
    assert torch.isfinite(dv).all() and float(dv[0].abs().max()) < 2.0 ** -90
    return p, dv


@pytest.mark.parametrize("vel_mode", [0, 1])
@pytest.mark.parametrize("model", ["terms/interior", "wrap"])
def test_prologue_per_element_against_fp64(cuda, cases, model, vel_mode):
    """dmax and oscale exactly, dam / ratio / dbeta per element within (roundings on the path) x 2^-24 of the fp64
    value, an exact zero where dv is zero; per-model magnitudes 2^-100, 1, 2^90 (a scale taken from another model
    is off by 2^90 at least; 2^90 is also past 2^63, where the scale's exponent is clamped at 126)."""
    p, dv = prologue_inputs(cases, model, vel_mode, cuda)
    zeros = check_workspace(p, dv, f"{model}/vel_mode{vel_mode}")
    assert zeros == {"dam": 3, "ratio": 1, "dbeta": 1}


@pytest.mark.parametrize("vel_mode", [0, 1])
def test_prologue_below_the_normal_range(cuda, cases, vel_mode):
    """The lower end of the scale's exponent (include/red_diffeq_fwi.h): a direction of denormals only (model 0,
    multiples of 2^-149 up to 1000) and a zero direction (model 1) are scaled by 2^63, oscale 2^-63; the scaled
    denormals are normal floats, so dam / ratio / dbeta meet the same bars, and the zero direction gives zeros.
    Model 2 is an ordinary direction."""
    p, dv = prologue_inputs(cases, "terms/interior", vel_mode, cuda)
    ints = np.random.default_rng(62).integers(-1000, 1001, size=tuple(dv[0].shape))
    denormal = (ints * 2.0 ** -149).astype(np.float32)               # exact: made in fp64 on the host, then copied
    dv[0] = torch.from_numpy(denormal).to(cuda)
    dv[1] = 0.0
    dv[2] = dv[2] * 2.0 ** -90
    back = dv[0].cpu().numpy()
    assert (back.astype(np.float64) * 2.0 ** 149 == ints).all() and 0 < np.abs(back).max() < 2.0 ** -126
    got = p.split(p.run(dv))
    assert (got["dmax"][:2] >> 23 == 0).all() and got["dmax"][1] == 0
    assert (got["oscale"][:2] == np.float32(2.0 ** -63)).all()
    zeros = check_workspace(p, dv, f"denormal/vel_mode{vel_mode}")
    assert zeros["dam"] >= p.nz * p.nx and zeros["ratio"] >= 1 and zeros["dbeta"] >= p.ns


@pytest.mark.parametrize("vel_mode", [0, 1])
def test_prologue_strides_and_dirty_workspace_bitwise(cuda, cases, vel_mode):
    """The same workspace bits from strided views of dv (the surroundings hold 1e30, which a wrong stride would
    bring into dmax), from a NaN-filled workspace, and from a workspace that served a direction 2^40 times larger
    just before (a stale dmax would show in oscale)."""
    p, dv = prologue_inputs(cases, "terms/interior", vel_mode, cuda)
    ref = p.run(dv)
    B, nz, nx = p.B, p.nz, p.nx
    frame = torch.full((B, 1, nz + 2, nx + 2), 1e30, device=cuda)
    frame[:, :, 1:-1, 1:-1] = dv
    view = frame[:, :, 1:-1, 1:-1]
    assert view.stride() == ((nz + 2) * (nx + 2), (nz + 2) * (nx + 2), nx + 2, 1)
    assert torch.equal(p.run(view), ref)
    chans = torch.full((B, 2, nz, nx), 1e30, device=cuda)
    chans[:, 1:2] = dv
    view = chans[:, 1:2]
    assert view.stride()[0] == 2 * nz * nx and view.data_ptr() != chans.data_ptr()
    assert torch.equal(p.run(view), ref)
    tr = dv.transpose(2, 3).contiguous().transpose(2, 3)              # column-major: s2 = 1, s3 = nz
    assert tr.stride()[2:] == (1, nz) and torch.equal(tr, dv)
    assert torch.equal(p.run(tr), ref)
    assert torch.equal(p.run(dv, p.new_work(float("nan"))), ref)
    small = dv * 2.0 ** -40
    work = p.new_work(float("nan"))
    assert torch.equal(p.run(dv, work), ref)
    again = p.run(small, work)
    fresh = p.run(small)
    assert torch.equal(again, fresh)
    a, f = p.split(again), p.split(ref)
    # model 1 (magnitude 1): the scale follows the direction, the scaled direction's bits do not change
    assert a["oscale"][1] == f["oscale"][1] * np.float32(2.0 ** -40)
    assert (a["dam"][1] == f["dam"][1]).all() and (a["dbeta"][1] == f["dbeta"][1]).all()


# ------------------------------------------------------------------------------------------ bitwise invariances
@pytest.fixture(scope="module")
def dense(cuda, cases):
    """The terms model with a dense direction: (case, fwi, dv, born(v, dv))."""
    c = cases["terms/interior"]
    fwi = c.fwi()
    dv = 0.04 * randn(c.v.shape, 71, cuda)
    ds = fwi.born(c.v, dv)
    fwi.check()
    assert float(ds[0].abs().max()) > 0 and float(ds[1].abs().max()) > 0
    return c, fwi, dv, ds


def test_per_model_scales_bitwise(cuda, dense):
    """born(v, s dv) = s born(v, dv) bit for bit with a different power of two per model (2^-30, 2^40): each
    model's scale comes from its own direction.  Both models of every other test have directions of one size."""
    c, fwi, dv, ds = dense
    s = torch.tensor([2.0 ** -30, 2.0 ** 40], device=cuda)[:, None, None, None]
    got = fwi.born(c.v, s * dv)
    assert same_bits(got, s * ds)
    assert same_bits(fwi.born(c.v, s.flip(0) * dv), s.flip(0) * ds)


def test_strided_model_and_direction_bitwise(cuda, dense):
    c, fwi, dv, ds = dense
    B, _, nz, nx = c.v.shape
    frame_v = torch.full((B, 1, nz + 2, nx + 2), float("nan"), device=cuda)
    frame_d = torch.full((B, 1, nz + 2, nx + 2), 1e30, device=cuda)
    frame_v[:, :, 1:-1, 1:-1], frame_d[:, :, 1:-1, 1:-1] = c.v, dv
    assert same_bits(fwi.born(frame_v[:, :, 1:-1, 1:-1], frame_d[:, :, 1:-1, 1:-1]), ds)
    chans_v = torch.full((B, 3, nz, nx), float("nan"), device=cuda)
    chans_d = torch.full((B, 2, nz, nx), 1e30, device=cuda)
    chans_v[:, 2:3], chans_d[:, 0:1] = c.v, dv
    assert same_bits(fwi.born(chans_v[:, 2:3], chans_d[:, 0:1]), ds)
    fwi.check()


def test_a_models_record_does_not_depend_on_the_other_direction(cuda, dense):
    """Model 1's record is the same bits whether model 0's direction is zero, another randn, 2^50 times larger or
    holds a NaN, and equals the B = 1 run; the same for model 0."""
    c, fwi, dv, ds = dense
    for keep in (1, 0):
        other = 1 - keep
        variants = {"zero": torch.zeros_like(dv[other]), "randn": 0.04 * randn(dv[other].shape, 72, cuda),
                    "large": dv[other] * 2.0 ** 50, "nan": dv[other].clone()}
        variants["nan"][0, 7, 9] = float("nan")
        for what, d in variants.items():
            mixed = dv.clone()
            mixed[other] = d
            got = fwi.born(c.v, mixed)
            assert same_bits(got[keep], ds[keep]), (keep, what)
            if what == "zero":
                assert torch.count_nonzero(got[other]) == 0
        one = c.fwi().born(c.v[keep:keep + 1].contiguous(), dv[keep:keep + 1].contiguous())
        assert same_bits(one[0], ds[keep]), keep
    fwi.check()


# ------------------------------------------------------------------------------------------ record length
def direct_launches(c):
    """(fwi, plan) of a case with graph capture off from the plan's first call on."""
    fwi = c.fwi()
    plan = fwi._plan(c.v.shape[2], c.v.shape[3], c.v.device)
    plan.set_graphs(False)
    return fwi, plan


@pytest.fixture(scope="module")
def wrap160(cuda, cases):
    c = cases["wrap"]
    return direct_launches(c)[0].born(c.v, c.dv)


@pytest.mark.parametrize("nt", [157, 158, 159, 161])
def test_record_length_tails_bitwise(cuda, cases, wrap160, nt):
    """nt = 160 leaves a tail at depth 3 only.  nt = 157 .. 161 leave tails of 1 .. 3 steps at depths 2, 3 and 4:
    every depth and chain count gives one record; it is the nt = 160 record on the samples both have (the wavelet's
    prefix does not depend on nt: tests/test_born_host.py, and a time step does not look ahead); and for nt <= 160
    it meets the per-model bar against the prefix of jdv64.
    Every call here is a direct launch (graph capture off).  Known fault, open: a Born call that captures a new graph
    for every depth and chain count, the [True] case of tests/test_gpu_born.py::test_schedule_independence_bitwise,
    has ended in a host segmentation fault once, cause unknown (Born section); this test does not add
    captures of that kind to the suite."""
    c = copy.copy(cases["wrap"])
    c.ctx = dict(c.ctx, nt=nt)
    fwi, plan = direct_launches(c)
    ref = fwi.born(c.v, c.dv)
    assert ref.shape == (c.v.shape[0], c.ctx["ns"], nt, c.ctx["ng"])
    for depth in (1, 2, 3, 4):
        for chains in (1, 3):
            plan.set_tuning(depth, depth, chains)
            assert same_bits(fwi.born(c.v, c.dv), ref), (nt, depth, chains)
    fwi.check()
    m = min(nt, 160)
    assert same_bits(ref[:, :, :m], wrap160[:, :, :m])
    if nt <= 160:
        err = rel_l2(ref, c.jdv64[:, :, :nt])
        for b, (e, eref) in enumerate(zip(err, c.eref)):
            record_margin("born_record_length_vs_fp64_over_4Eref", f"wrap nt {nt}[{b}]", e, 4 * eref)
        assert (err <= 4 * c.eref).all(), (nt, err, c.eref)


# ------------------------------------------------------------------------------------------ graph replays
def test_born_graph_replays_on_poisoned_buffers(cuda, dense):
    """Cached-graph replays of the Born time loop (graph kind 5) behind its prologue on a fixed workspace, ring and
    record that are NaN-filled before every call: each call must zero what it starts from (dmax, the ring's first
    two levels) and equal the direct launches bit for bit (the pattern of
    tests/test_gpu_fwi.py::test_chunked_graph_replays_on_poisoned_buffers)."""
    from red_diffeq import _hip
    c, _, dv, ds = dense
    fwi = c.fwi()
    B = c.v.shape[0]
    plan = fwi._plan(c.v.shape[2], c.v.shape[3], c.v.device)
    sz = plan.sizes(B)
    coeffs, vstat = plan.coeffs(c.v, 0)
    _, hist = plan.forward(coeffs, B, True)
    nbytes = ctypes.c_size_t()
    _hip.check(plan.lib.rdq_fwi_born_sizes(plan.handle, B, ctypes.byref(nbytes)), "rdq_fwi_born_sizes")
    f32 = lambda n: torch.empty(int(n) // 4, device=cuda)
    dwork, ring = f32(nbytes.value), f32(sz.ring)
    dseis = torch.empty(B, plan.ns, sz.nrec, plan.ng, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    strides = (ctypes.c_int64 * 4)(*dv.stride())
    P = _hip.ptr

    def run():
        for t in (dwork, ring, dseis):
            t.fill_(float("nan"))
        _hip.check(plan.lib.rdq_fwi_dcoeffs(plan.handle, B, P(dv), strides, 0, P(coeffs), P(vstat), P(dwork), st),
                   "rdq_fwi_dcoeffs")
        _hip.check(plan.lib.rdq_fwi_born(plan.handle, B, P(coeffs), P(dwork), P(hist), P(dseis), P(ring), st),
                   "rdq_fwi_born")
        torch.cuda.synchronize()
        return dseis.clone()

    plan.set_graphs(False)
    want = run()
    assert same_bits(want, ds)
    plan.set_graphs(True)
    for rep in range(3):                  # capture, then two replays of the same graph exec
        assert same_bits(run(), want), rep
    fwi.check()
