"""Host side of prior sampling: the DDIM schedule against the reference's own (time, time_next) pairs and step
scalars (tests/golden/make_sampling.py reads them out of the reference's ddim_sample), the sample() dispatch, and
the argument checks of rdq_sample_step, which return before any HIP call.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from red_diffeq import _hip
from red_diffeq.models.diffusion import GaussianDiffusion, ddim_schedule

INVALID = -10001


class _Net(torch.nn.Module):
    channels, out_dim, self_condition = 1, 1, False


def _diffusion(**kw):
    return GaussianDiffusion(_Net(), image_size=72, objective=kw.pop("objective", "pred_noise"), **kw)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("sampling_dim8")


@pytest.mark.parametrize("S", [6, 250])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_schedule_is_the_references(fixture, S, eta):
    """pairs exactly; sqrt(alpha_next), c and sigma bit for bit (fp32 torch expressions on the CPU tables)."""
    d = _diffusion(timesteps=1000, sampling_timesteps=S, ddim_sampling_eta=eta)
    pairs, coef = ddim_schedule(d.alphas_cumprod, d.num_timesteps, S, eta)
    tag = f"sched_S{S}_eta{int(eta)}"
    assert len(pairs) == S and pairs == [tuple(p) for p in fixture[tag + "_pairs"].tolist()]
    assert coef.dtype == torch.float32 and coef.shape == (S, 3)
    want = fixture[tag + "_coef"]
    assert want.shape == (S - 1, 3)
    assert np.array_equal(coef[:-1].numpy().view(np.int32), want.view(np.int32))
    assert pairs[-1][1] == -1 and not coef[-1].any()
    if eta == 0.0:
        assert not coef[:, 2].any()
    else:
        assert (coef[:-1, 2] > 0).all()


@pytest.mark.parametrize("tag,S,eta,objective", [("ddim0", 6, 0.0, "pred_noise"), ("ddim1", 6, 1.0, "pred_noise"),
                                                 ("ddim_v", 3, 0.0, "pred_v")])
def test_ddim_schedule_of_the_sampling_cases(fixture, tag, S, eta, objective):
    d = _diffusion(timesteps=1000, sampling_timesteps=S, ddim_sampling_eta=eta, objective=objective)
    pairs, coef = d._ddim_schedule()
    assert pairs == [tuple(p) for p in fixture[tag + "_pairs"].tolist()]
    assert np.array_equal(coef[:-1].numpy().view(np.int32), fixture[tag + "_coef"].view(np.int32))
    assert d._ddim_schedule()[1] is coef                      # kept: no second fetch of alphas_cumprod
    d.ddim_sampling_eta = 0.5
    assert d._ddim_schedule()[1] is not coef


def test_sample_dispatches_on_is_ddim_sampling():
    calls = []
    for kw, want in ((dict(timesteps=8), "anc"), (dict(timesteps=8, sampling_timesteps=4), "ddim")):
        d = _diffusion(**kw)
        d.p_sample_loop = lambda shape, **k: calls.append(("anc", tuple(shape), k))
        d.ddim_sample = lambda shape, **k: calls.append(("ddim", tuple(shape), k))
        g = torch.Generator()
        d.sample(batch_size=3, return_all_timesteps=True, generator=g)
        name, shape, k = calls.pop()
        assert name == want and shape == (3, 1, 72, 72) and not calls
        assert k == dict(return_all_timesteps=True, generator=g, noise=None)


def test_sampling_methods_keep_the_reference_signatures():
    import inspect
    d = _diffusion(timesteps=8)
    sig = {n: list(inspect.signature(getattr(d, n)).parameters) for n in
           ("p_sample", "p_sample_loop", "ddim_sample", "sample", "interpolate")}
    assert sig["p_sample"][:3] == ["x", "t", "x_self_cond"]
    assert sig["p_sample_loop"][:3] == ["shape", "return_all_timesteps", "plot_show"]
    assert sig["ddim_sample"][:2] == ["shape", "return_all_timesteps"]
    assert sig["sample"][:2] == ["batch_size", "return_all_timesteps"]
    assert sig["interpolate"][:4] == ["x1", "x2", "t", "lam"]
    for n, names in sig.items():
        assert names[-2:] == ["generator", "noise"], n
        kinds = inspect.signature(getattr(d, n)).parameters
        assert all(kinds[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("generator", "noise")), n


# ------------------------------------------------------------------------------- rdq_sample_step rejections
P = ctypes.c_void_p(64)       # never dereferenced: every case is rejected before a launch


def _call(**changes):
    tab = {n: P for n, _ in _hip.SampleTables._fields_}
    a = dict(B=2, n=5184, objective=0, mode=1, T=1000, t=P, x_t=P, out=P, noise=P, a_next=0.5, c=0.5, sigma=0.1,
             t_next=10, x_next=P, x_start_out=None, t_out=None)
    for k, v in changes.items():
        if k in tab:
            tab[k] = v
        else:
            a[k] = v
    tables = None if changes.get("tables", 1) is None else ctypes.byref(_hip.SampleTables(**tab))
    a.pop("tables", None)
    return _hip.load_library().rdq_sample_step(a["B"], a["n"], a["objective"], a["mode"], a["T"], tables, a["t"],
                                               a["x_t"], a["out"], a["noise"], a["a_next"], a["c"], a["sigma"],
                                               a["t_next"], a["x_next"], a["x_start_out"], a["t_out"], None)


REJECTED = [dict(B=0), dict(B=65536), dict(n=0), dict(T=0), dict(tables=None), dict(t=None), dict(x_t=None),
            dict(out=None), dict(x_next=None), dict(objective=-1), dict(objective=3), dict(mode=-1), dict(mode=3),
            dict(t_next=1000),
            dict(sqrt_recip_ac=None), dict(sqrt_recipm1_ac=None),                       # pred_noise / DDIM
            dict(objective=2, sqrt_ac=None), dict(objective=2, sqrt_1mac=None),          # pred_v
            dict(mode=0, post_coef1=None), dict(mode=0, post_coef2=None), dict(mode=0, post_logvar=None),
            dict(noise=None),                                                            # DDIM, sigma != 0
            dict(t_out=P),                                                               # t_out is t
            dict(x_start_out=P)]                                                         # x_start_out is x_t


@pytest.mark.parametrize("changes", REJECTED, ids=[",".join(f"{k}={v if not isinstance(v, ctypes.c_void_p) else 'same'}"
                                                            for k, v in c.items()) for c in REJECTED])
def test_sample_step_rejects(changes):
    """One invalid argument, everything else valid: RDQ_E_INVALID, before any HIP call."""
    assert _call(**changes) == INVALID
