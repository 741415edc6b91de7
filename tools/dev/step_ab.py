"""Developer script (GPU box): every output of every step entry point of one build of the library, at small shapes, into an .npz -- run it on
two builds and compare the files array by array (numpy.array_equal) to show that a host-side change moved no result.

    python tools/dev/step_ab.py --lib PATH --out FILE.npz
    python tools/dev/step_ab.py --compare A.npz B.npz

Entry points (B 5, k 3 unless said; scalars, every `want` tensor, the gradient, parameters and Adam moments after three steps): forward;
forward_backward; forward_backward_split (offset and gradient); train_step with and without tensors; the three masked calls on a 50 % mask;
train_step_dataset without and with resident masks; grad_moments B 20, k 5, M 4; eval_llh N 7, k 50.  Models: 1-layer 64/8/48, 2-layer
[64, 32]/[8, 4]/48 (no masked calls: the masked step is the 1-layer model's), both precisions, and the masked calls once more on a bf16
1-layer handle whose hidden width 50 pads to 64; the images once as a host array and once as a device pointer.  One child process per
precision, each under its own `timeout`; the script stops at the first child that does not exit with 0.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
ap.add_argument("--child", choices=("bf16", "fp32"), help="(internal) the calls of one precision, in this process")
args = ap.parse_args()

if args.compare:
    a, b = (np.load(p) for p in args.compare)
    keys = sorted((set(a.files) | set(b.files)) - {"build_id"})
    bad = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    print("build ids: %s | %s" % (a["build_id"], b["build_id"]))
    print("%d arrays, %d differ%s" % (len(keys), len(bad), "".join("\n  " + k for k in bad)))
    sys.exit(1 if bad else 0)

if not args.child:
    out = {}
    for prec in ("bf16", "fp32"):
        part = "%s.%s.npz" % (args.out, prec)
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", prec, "--out", part] + (["--lib", args.lib] if args.lib else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print("FAILED (exit %d): %s" % (rc, " ".join(cmd)))
            sys.exit(1)
        with np.load(part) as z:
            out.update({k: z[k] for k in z.files})
        os.remove(part)
    np.savez(args.out, **out)
    print("build %s: %d arrays -> %s" % (out["build_id"], len(out) - 1, args.out))
    sys.exit(0)

from iwae_amd import _capi
if args.lib:
    _capi.LIB_PATH = os.path.abspath(args.lib)
import ctypes as C
import torch
from iwae_amd._capi import Scalars, check
from iwae_amd.native import NativeModel, _SCALAR_NAMES


def on_host(a):
    """(owner, address) of a float32 array in host memory"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data


def on_device(a):
    """... and of a copy of it on the device"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t, t.data_ptr()


def step_call(m, name, xp, k, tail, want=(), mask=None):
    """iwae_<name> or, with a mask, iwae_<name>_masked through the C ABI on the address xp of B images: scalars and the `want` tensors"""
    t, bufs = m._want(want, B, k)
    s = Scalars()
    head = (m.h, C.c_void_p(xp)) + ((mask.ctypes.data,) if mask is not None else ())
    check(getattr(m.lib, "iwae_" + name + ("_masked" if mask is not None else ""))(*head, B, k, *tail, None, C.byref(s), C.byref(t) if t is not None else None))
    r = {n: float(getattr(s, n)) for n in _SCALAR_NAMES}
    r.update(bufs)
    return r


out = {"build_id": np.array(_capi.library_build_id())}
B, K, XD = 5, 3, 48
OBJ = _capi.OBJECTIVES["iwae_elbo"]
ROWS = ("lpxz", "lpz", "lqzx", "lpz2", "lqzx2", "log_w", "al", "z", "z2", "snis_z", "snis_z2")      # (NativeModel drops the 2-layer names on a 1-layer handle)
rng = np.random.default_rng(17)
X = (rng.random((20, XD)) < 0.4).astype(np.float32)
MASK = rng.random((20, XD)) < 0.5
GRAY = rng.integers(0, 256, (12, XD)).astype(np.uint8)


def keep(tag, r):
    if isinstance(r, dict):
        for k, v in r.items():
            keep("%s.%s" % (tag, k), v)
    elif isinstance(r, (list, tuple)):
        for i, v in enumerate(r):
            keep("%s.%d" % (tag, i), v)
    else:
        out[tag] = np.asarray(r).copy()


def keep_state(tag, m, grads=False):
    if grads:
        keep(tag + ".grads", m.get_grads())
    else:
        keep(tag + ".params", m.get_params())
        keep(tag + ".adam", m.get_adam_state())


def run(tag, prec, put, layers, nh, nl, masked_only=False):
    m = NativeModel(layers, nh, nl, x_dim=XD, seed=123, precision=prec)
    m.set_eval_precision(prec)
    p0, zero = m.get_params().copy(), np.zeros(m.n_params, np.float32)
    x, xp = put(X[:B])

    def reset(step):
        m.set_params(p0)
        m.set_adam_state(zero, zero, 0)
        m.set_step(step, 2)

    if not masked_only:
        reset(3)
        keep(tag + "forward", step_call(m, "forward", xp, K, (1.0,), ROWS + ("logits",)))
        reset(4)
        keep(tag + "forward_backward", step_call(m, "forward_backward", xp, K, (1.0, OBJ), ROWS + ("logits",)))
        keep_state(tag + "forward_backward", m, grads=True)
        reset(5)
        keep(tag + "split.offset", m.forward_backward_split_devptr(xp, B, K, 1.0, OBJ)[1])
        keep_state(tag + "split", m, grads=True)
        reset(6)
        for i in range(3):
            keep(tag + "train_tensors.%d" % i, step_call(m, "train_step", xp, K, (1.0, 1e-3, OBJ), ROWS + ("logits",)))
        keep_state(tag + "train_tensors", m)
        reset(7)
        for i in range(3):
            keep(tag + "train.%d" % i, step_call(m, "train_step", xp, K, (1.0, 1e-3, OBJ)))
        keep_state(tag + "train", m)
    if layers == 1:
        mk = np.ascontiguousarray(MASK[:B], dtype=np.uint8)
        reset(8)
        keep(tag + "forward_masked", step_call(m, "forward", xp, K, (1.0,), ROWS, mk))
        reset(9)
        keep(tag + "forward_backward_masked", step_call(m, "forward_backward", xp, K, (1.0, OBJ), ROWS, mk))
        keep_state(tag + "forward_backward_masked", m, grads=True)
        reset(10)
        for i in range(3):      # (the first step hands out tensors: both ends of the masked train step)
            keep(tag + "train_masked.%d" % i, step_call(m, "train_step", xp, K, (1.0, 1e-3, OBJ), ROWS if i == 0 else (), mk))
        keep_state(tag + "train_masked", m)
    if not masked_only:
        m.dataset_upload(GRAY)
        for name in ("dataset", "dataset_masked"):
            if name == "dataset_masked":
                if layers != 1:
                    continue
                m.dataset_mcar_mask(0.5, 99)
            reset(11)
            m.dataset_begin_epoch(1)
            for i in range(3):
                keep(tag + "%s.%d" % (name, i), m.train_step_dataset(3 * i, B, K))
            keep_state(tag + name, m)
        m.dataset_set_mask(None)
        reset(12)
        x20, x20p = put(X[:20])
        mean, var = np.empty(m.n_params, np.float64), np.empty(m.n_params, np.float64)
        m.grad_moments_devptr(x20p, 20, 5, 4, 1.0, OBJ, mean.ctypes.data, var.ctypes.data)
        keep(tag + "grad_moments", (mean, var))
        reset(13)
        x7, x7p = put(X[:7])
        llh, per_image = C.c_double(), np.empty(7, np.float32)
        check(m.lib.iwae_eval_llh(m.h, C.c_void_p(x7p), 7, 50, 0, C.byref(llh), per_image.ctypes.data))
        keep(tag + "eval_llh", (llh.value, per_image))
    m.close()


prec = args.child
for where, put in (("host", on_host), ("dev", on_device)):
    run("%s.%s.one." % (prec, where), prec, put, 1, [64], [8])
    run("%s.%s.two." % (prec, where), prec, put, 2, [64, 32], [8, 4])
    if prec == "bf16":
        run("%s.%s.pad64." % (prec, where), prec, put, 1, [50], [8], masked_only=True)
np.savez(args.out, **out)
print("build %s (%s): %d arrays -> %s" % (out["build_id"], prec, len(out) - 1, args.out))
