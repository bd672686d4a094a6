"""Shared by tests/test_encoding_host.py and tests/test_gpu_encoding.py: the cases of tests/golden/encoding.npz
(tests/golden/make_encoding.py): fp64 truth of encoded supershots, built from per-shot reference runs by linearity,
and the reference's own fp32 errors as yardsticks."""
import numpy as np

from conftest import load_golden

CASES = ("wrap", "tiles", "geom", "short", "shared")


class Fixture:
    def __init__(self, tag):
        z = load_golden("encoding")
        pre = f"{tag}_ctx_"
        self.ctx = {k[len(pre):]: (z[k].item() if z[k].ndim == 0 else z[k].tolist()) for k in z.files
                    if k.startswith(pre)}
        self.tag, self.normalize, self.st = tag, bool(z[f"{tag}_normalize"]), int(z[f"{tag}_st"])
        for name in ("v", "W", "E", "r", "seis64", "eref", "gv64", "gW64", "gE64", "eref_v", "eref_w", "eref_E",
                     "dW", "ip"):
            setattr(self, name, z[f"{tag}_{name}"])
        self.B, self.ns, self.nt = self.W.shape
        self.ne = self.E.shape[0]
        # the codes of make_encoding.py as row ranges of E: the supershots of a call are independent of each other, so
        # a call with a row subset is compared with the same rows of the truth
        self.codes = {"all (ne > ns)": slice(0, self.ne), "sign": slice(0, 2),
                      "gaussian with a zero": slice(2, self.ne), "ne = 1": slice(0, 1)}

    def fwi(self, device="cuda", **kw):
        from red_diffeq.solvers.pde import FWIForward
        from red_diffeq.utils.data_trans import s_normalize_none, v_denormalize
        if self.normalize:
            kw = dict(dict(v_denorm_func=v_denormalize, s_norm_func=s_normalize_none), **kw)
        return FWIForward(dict(self.ctx), device, sample_temporal=self.st, normalize=self.normalize, **kw)
