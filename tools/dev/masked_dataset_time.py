"""Developer script (GPU box): the masked train step fed from the resident data set at section 20's timing workload --
the 1-layer model at the reference's dims (784 / 200 / 100), k = 50, a 50 % completely-at-random mask, device noise -- interleaved in one
process, per precision, with the three steps it is read against:
  (a) resident_masked   iwae_train_step_dataset on a handle with iwae_dataset_mcar_mask: gather, binarisation and every masked form of the
                        rows in ONE input kernel (gather_binarize_masked_kernel), no host traffic
  (b) devptr_masked     iwae_train_step_masked on pre-gathered, pre-binarised x and mask resident on the device: the fastest masked route
                        before the resident masks; it leaves out the gather and the binarisation, so it is a floor for the old way
  (c) host_fed          tasks/miwae.py's loop without --resident: NumPy indexing X[idx], mask[idx] and an upload per step
  (d) resident_unmasked iwae_train_step_dataset without masks (the flagship input path)
Four handles take turns, ROUNDS rounds of STEPS steps each, synchronised around each block; printed per batch size are the median and the
spread of the per-step times over the rounds, the condition (a) <= (b) (1 + s) with s = (b)'s own spread (max - min) / median, and the
ratios (a)/(c) and (a)/(d) as found.  One GPU process; run it under a time limit.

    python tools/dev/masked_dataset_time.py [rounds] [steps] [B ...]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel, OBJECTIVES

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
BATCHES = [int(v) for v in sys.argv[3:]] or [1024, 164, 328, 512, 800, 2048]
K, H, D, X = 50, 200, 100, 784
N = 16384                     # images of the resident set
obj = OBJECTIVES["iwae_elbo"]
NAMES = ("resident_masked", "devptr_masked", "host_fed", "resident_unmasked")

gray = np.clip(np.rint(utils.synthetic_mnist(n_train=N, n_test=1)[0] * 255.0), 0, 255).astype(np.uint8)
host_mask = utils.device_mcar_mask(N, X, 0.5, 2)
host_x = (np.random.default_rng(0).random(gray.shape) < gray / 255.0).astype(np.float32)      # (c): one fixed binarisation, as tasks/miwae.py trains

for prec in ("bf16", "fp32"):
    models = {}
    for name in NAMES:
        m = NativeModel(1, H, D, seed=5, precision=prec)
        m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
        if name.startswith("resident"):
            m.dataset_upload(gray)
            m.dataset_begin_epoch(1, np.random.default_rng(1).permutation(N).astype(np.int32))
        if name == "resident_masked":
            m.dataset_mcar_mask(0.5, 2)
        models[name] = m
    for B in BATCHES:
        x = torch.tensor(O.synthetic_binarized(B, 1), device="cuda")
        mask = torch.tensor(host_mask[:B], device="cuda")
        nb = N // B
        rng = np.random.default_rng(3)
        pos = {"i": 0}

        def block(name, steps):
            m = models[name]
            m.sync()
            t = time.perf_counter()
            for _ in range(steps):
                if name == "devptr_masked":
                    m.train_step_masked_devptr(x.data_ptr(), mask.data_ptr(), B, K, 1.0, 1e-3, obj)
                elif name == "host_fed":
                    idx = rng.choice(N, size=B, replace=False)
                    m.train_step(host_x[idx], K, 1.0, 1e-3, "iwae_elbo", mask=host_mask[idx])
                else:
                    pos["i"] = (pos["i"] + 1) % nb
                    m.train_step_dataset(pos["i"] * B, B, K, 1.0, 1e-3, "iwae_elbo", scalars=False)
            m.sync()
            return (time.perf_counter() - t) / steps

        for name in NAMES:
            block(name, 10)          # (warm-up: module load, the buffers grow)
        times = {name: [] for name in NAMES}
        for _ in range(ROUNDS):
            for name in NAMES:
                times[name].append(block(name, STEPS))
        print("# %s, B = %d, k = %d (%d rows), %d / %d / %d, iwae_elbo; %d rounds of %d steps, interleaved" % (prec, B, K, B * K, X, H, D, ROUNDS, STEPS))
        for name, ts in times.items():
            print("%-17s median %.4f ms per step  (min %.4f, max %.4f)" % (name, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3))
        med = {name: statistics.median(ts) for name, ts in times.items()}
        tb = times["devptr_masked"]
        s = (max(tb) - min(tb)) / med["devptr_masked"]
        bound = med["devptr_masked"] * (1.0 + s)
        print("resident_masked <= devptr_masked (1 + s): %.4f vs %.4f ms (s = %.4f): %s   resident_masked / host_fed = %.3f   / resident_unmasked = %.3f"
              % (med["resident_masked"] * 1e3, bound * 1e3, s, "holds" if med["resident_masked"] <= bound else "DOES NOT HOLD",
                 med["resident_masked"] / med["host_fed"], med["resident_masked"] / med["resident_unmasked"]), flush=True)
    for m in models.values():
        m.close()
