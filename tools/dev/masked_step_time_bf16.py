"""Developer script (GPU box): the masked train step on a bf16 handle at the masked step's timing workload -- binarised
images, k = 50, the 1-layer model at the reference's dims (784 / 200 / 100), a 50 % completely-at-random mask, x and the mask resident on the
device, device noise -- interleaved in one process with the three steps it is read against:
  (a) masked_bf16       iwae_train_step_masked on a bf16 handle: the hole-aware dense_kernel<EPI_BERN> behind dense_kernel / block_fwd_kernel
  (b) masked_f32        iwae_train_step_masked on a float32 handle at its default options (masked_step_time.py's step)
  (c) unmasked_bf16     iwae_train_step on a bf16 handle at its default plan (bern_pipe_kernel: the flagship step)
  (d) unmasked_same     iwae_train_step on a bf16 handle under no_bern_pipe + no_out_in_block: (a)'s kernels without holes
Four handles take turns, ROUNDS rounds of STEPS steps each, synchronised around each block; printed per batch size are the median and the
spread of the per-step times over the rounds and the ratios (a)/(b) -- the condition: below 1 at B = 1 024 --, (a)/(d) -- the price of the
hole test in the epilogue, the code kernel and the mask pass -- and (a)/(c) -- what a masked bern_pipe_kernel could still win.  One GPU
process; run it under a time limit.

    python tools/dev/masked_step_time_bf16.py [rounds] [steps] [B ...]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel, OBJECTIVES

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
BATCHES = [int(v) for v in sys.argv[3:]] or [1024, 164, 328, 512, 800, 2048]
K, H, D, X = 50, 200, 100, 784
obj = OBJECTIVES["iwae_elbo"]
handles = {"masked_bf16": ("bf16", {}, True), "masked_f32": ("fp32", {}, True), "unmasked_bf16": ("bf16", {}, False),
           "unmasked_same": ("bf16", {"no_bern_pipe": 1, "no_out_in_block": 1}, False)}
models = {}
for name, (prec, opts, _) in handles.items():
    m = NativeModel(1, H, D, seed=5, precision=prec, options=opts)
    m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
    models[name] = m

for B in BATCHES:
    x = torch.tensor(O.synthetic_binarized(B, 1), device="cuda")
    mask = torch.tensor(utils.mcar_mask((B, X), 0.5, seed=2), device="cuda")

    def block(name, steps):
        m = models[name]
        m.sync()
        t = time.perf_counter()
        for _ in range(steps):
            if handles[name][2]:
                m.train_step_masked_devptr(x.data_ptr(), mask.data_ptr(), B, K, 1.0, 1e-3, obj)
            else:
                m.train_step_devptr(x.data_ptr(), B, K, 1.0, 1e-3, obj)
        m.sync()
        return (time.perf_counter() - t) / steps

    for name in models:
        block(name, 10)          # (warm-up: module load, the buffers grow)
    times = {name: [] for name in models}
    for _ in range(ROUNDS):
        for name in models:
            times[name].append(block(name, STEPS))
    print("# B = %d, k = %d (%d rows), %d / %d / %d, iwae_elbo; %d rounds of %d steps, interleaved" % (B, K, B * K, X, H, D, ROUNDS, STEPS))
    for name, ts in times.items():
        print("%-15s median %.4f ms per step  (min %.4f, max %.4f)" % (name, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    print("masked_bf16 / masked_f32 = %.3f   / unmasked_same = %.3f   / unmasked_bf16 = %.3f"
          % (med["masked_bf16"] / med["masked_f32"], med["masked_bf16"] / med["unmasked_same"], med["masked_bf16"] / med["unmasked_bf16"]), flush=True)
for m in models.values():
    m.close()
