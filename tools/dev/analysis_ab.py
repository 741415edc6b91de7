"""Developer script (GPU box): every output of every evaluation call of one build of the library, at small shapes, into an .npz -- run it on
two builds and compare the files array by array (numpy.array_equal) to show that a host-side change moved no result.

    python tools/dev/analysis_ab.py --lib PATH --out FILE.npz
    python tools/dev/analysis_ab.py --compare A.npz B.npz

Calls (both precisions; the images once as a host array, once as a device pointer): grid_posterior 64/2/48 N=5 G=1500 in two chunks with
log_joint; latent_activity N=3 k=200 on the small and the reference 2-layer models; aggregate_posterior 64/8/48 N=37 S=3 with the
per-sample outputs; ais 64/8/48 N=3 C=7 T=6 L=2 with trace from both inits; local_posterior 64/8/48 N=3 S=5 T=4 E=2 with trace, once on
the caller's draws and once on Philox; impute 64/8/48 under a 50 % mask at N=5 S=3 (several images per workgroup, a dead row), N=2 S=70 (two
chunks per image and impute_merge_kernel) and N=5 S=3 without a mask; grad_moments B=20 k=5 M=4; eval_llh N=7 k=50; decode n=5.
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
args = ap.parse_args()

if args.compare:
    a, b = (np.load(p) for p in args.compare)
    keys = sorted((set(a.files) | set(b.files)) - {"build_id"})
    bad = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    print("build ids: %s | %s" % (a["build_id"], b["build_id"]))
    print("%d arrays, %d differ%s" % (len(keys), len(bad), "".join("\n  " + k for k in bad)))
    sys.exit(1 if bad else 0)

from iwae_amd import _capi
if args.lib:
    _capi.LIB_PATH = os.path.abspath(args.lib)
import torch
from oracle import iwae_np as O
import make_golden as MG
import iwae_amd.native as native
from iwae_amd.native import NativeModel


class DevArray:
    """A float32 array on the device, dressed as numpy just enough for NativeModel's wrappers (shape, reshape, ctypes.data)."""
    def __init__(self, a):
        self.t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        self.shape = a.shape
        self.ctypes = types.SimpleNamespace(data=self.t.data_ptr())

    def reshape(self, *shape):
        return self


_host_f32 = native._f32
native._f32 = lambda a: a if isinstance(a, DevArray) else _host_f32(a)

out = {"build_id": np.array(_capi.library_build_id())}


def keep(tag, r):
    if isinstance(r, dict):
        for k, v in r.items():
            keep("%s.%s" % (tag, k), v)
    elif isinstance(r, (list, tuple)):
        for i, v in enumerate(r):
            keep("%s.%d" % (tag, i), v)
    else:
        out[tag] = np.asarray(r)


def model(layers, nh, nl, xd, N, seed, prec, **kw):
    x, P, _ = MG.inputs(layers, nh, nl, xd, N, 1, seed)
    m = NativeModel(layers, nh, nl, x_dim=xd, seed=123, precision=prec, **kw)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision(prec)
    return m, x


rng = np.random.default_rng(5)
z = rng.uniform(-3.0, 3.0, (1500, 2)).astype(np.float32)
lw = rng.uniform(-1.0, 0.0, 1500).astype(np.float32)
lq_noise = rng.standard_normal((4 + 2, 5, 3, 8)).astype(np.float32)
im_mask = rng.random((5, 48)) < 0.5
for prec in ("fp32", "bf16"):
    for where in ("host", "dev"):
        put = (lambda a: a) if where == "host" else DevArray
        tag = "%s.%s." % (prec, where)
        m, x = model(1, 64, 2, 48, 5, 31, prec, options={"grid_chunk": 1024})
        m.set_step(3, 1)
        keep(tag + "grid", m.grid_posterior(put(x), z, lw, log_joint=True))
        m.close()
        for name, (nh, nl, xd) in (("small2", ([64, 32], [16, 8], 48)), ("ref2", ([200, 100], [100, 50], 784))):
            m, x = model(2, nh, nl, xd, 3, 33, prec)
            m.set_step(4, 2)
            keep(tag + "activity." + name, m.latent_activity(put(x), k=200, per_image=True))
            m.close()
        m, x = model(1, 64, 8, 48, 37, 35, prec)
        m.set_step(5, 3)
        keep(tag + "aggregate", m.aggregate_posterior(put(x), n_samples=3, per_sample=True))
        for init in ("encoder", "prior"):
            m.set_step(6, 4)
            keep(tag + "ais." + init, m.ais(put(x[:3]), n_chains=7, n_temps=6, leapfrog=2, init=init, trace=True))
        m.set_step(9, 6)
        keep(tag + "local_q.noise", m.local_posterior(put(x[:3]), n_samples=5, n_iters=4, n_eval=2, noise=lq_noise, trace=True))
        keep(tag + "local_q.philox", m.local_posterior(put(x[:3]), n_samples=5, n_iters=4, n_eval=2, trace=True))
        m.set_step(10, 7)
        keep(tag + "impute.s3", m.impute(put(x[:5]), mask=im_mask, n_samples=3))
        keep(tag + "impute.s70", m.impute(put(x[:2]), mask=im_mask[:2], n_samples=70))
        keep(tag + "impute.nomask", m.impute(put(x[:5]), n_samples=3))
        m.set_step(7, 0)
        keep(tag + "grad_moments", m.grad_moments(put(x[:20]), 5, 4))
        m.set_step(8, 5)
        keep(tag + "eval_llh", m.eval_llh(put(x[:7]), k=50, per_image=True))
        keep(tag + "decode", m.decode(rng.standard_normal((5, 8)).astype(np.float32)))
        m.close()
np.savez(args.out, **out)
print("build %s: %d arrays -> %s" % (out["build_id"], len(out) - 1, args.out))
