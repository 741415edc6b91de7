"""Training on incomplete images (Mattei & Frellsen 2019, MIWAE): every training image gets one fixed missing-completely-at-random mask
and a 1-layer model is trained (--precision fp32, the default, or bf16: the bf16 MFMA step) on the (x, mask) batches with the masked train step (IWAE.train_step(..., mask=...)): the
encoder sees the observed pixels, the bound is that on log p(x_obs).  Beside it the same model trained on the same images with the holes
filled by zeros and no mask -- what one can do without the masked step.  Reported for both, on held-out images masked at the same rate
through IWAE.impute: the mean k-draw bound on log p(x_obs), and on the UNOBSERVED pixels the Bernoulli cross-entropy and the mean absolute
error of the imputation.  Same flags as main.py, plus --images, --test-images, --steps, --rate, --draws, --mask-seed, --lr,
--precision, --resident.

--resident trains both models through the device-resident data pipeline instead of host batches of one fixed
binarisation: the grey levels stay in HBM, every epoch gets a visiting order and a fresh dynamic binarisation, and the masked model's masks
ride along (IWAE.set_dataset(gray, mask) + train_step_dataset); the zero-filled model trains on gray * (mask != 0) without a mask -- a grey
level of 0 binarises to 0 at every epoch.

    python tasks/miwae.py --n_samples 5 --objective iwae_elbo --images 10000 --steps 2000 --rate 0.5
"""
import argparse

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
from iwae_amd import iwae1, utils
from iwae_amd.optimizers import Adam


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the masks' and the run's."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--images", type=int, default=10000, help="training images")
    p.add_argument("--test-images", type=int, default=1000, help="held-out images the two models are scored on")
    p.add_argument("--steps", type=int, default=2000, help="train steps per model")
    p.add_argument("--rate", type=float, default=0.5, help="fraction of the pixels hidden, completely at random")
    p.add_argument("--draws", type=int, default=50, help="importance draws per image of the evaluation (1..65536)")
    p.add_argument("--mask-seed", type=int, default=0, help="seed of the masks")
    p.add_argument("--lr", type=float, default=1e-3, help="Adam's learning rate")
    # (no attribute unless given: the namespace of a run without the flag is what it was before the flag existed; precision_of reads it)
    p.add_argument("--precision", choices=("fp32", "bf16"), default=argparse.SUPPRESS,
                   help="arithmetic of both models' train steps: fp32 (the default) or bf16 (bf16 operands, float32 accumulation)")
    p.add_argument("--resident", action="store_true", default=argparse.SUPPRESS,
                   help="train from the device-resident grey-level set with per-epoch binarisation (masks resident too), not from host batches")
    return p


def precision_of(args):
    return getattr(args, "precision", "fp32")


def resident_of(args):
    return bool(getattr(args, "resident", False))


def load_gray(n_train, n_test):
    """Grey-level images [n, 784] in [0, 1] (local MNIST or the synthetic stand-in)."""
    data = utils.load_mnist()
    if data is not None:
        tr, te = data[0][0].reshape(-1, 784) / 255.0, data[1][0].reshape(-1, 784) / 255.0
    else:
        tr, te = utils.synthetic_mnist(n_train=n_train, n_test=n_test)[:2]
    return np.asarray(tr)[:n_train], np.asarray(te)[:n_test]


def load_images(n_train, n_test, seed=0):
    """Binarised images [n, 784] float32 (local MNIST or the synthetic stand-in), one fixed binarisation."""
    tr, te = load_gray(n_train, n_test)
    rng = np.random.default_rng(seed)
    return (rng.random(tr.shape) < tr).astype(np.float32), (rng.random(te.shape) < te).astype(np.float32)


def scores(x, p, hidden):
    """Bernoulli cross-entropy (nats per pixel) and mean absolute error of the probabilities p against x over the `hidden` pixels."""
    x, p = np.asarray(x, dtype=np.float64)[hidden], np.clip(np.asarray(p, dtype=np.float64)[hidden], 1e-7, 1.0 - 1e-7)
    return float(np.mean(-(x * np.log(p) + (1.0 - x) * np.log1p(-p)))), float(np.mean(np.abs(x - p)))


def train(args, X, mask, masked, seed=123):
    """A 1-layer model (--precision) trained for args.steps steps on batches of X: masked, on (x, mask); else on the zero-filled images.
    Returns (model, the objective's value at every step)."""
    seen = (mask != 0).astype(np.float64)      # the output bias: each pixel's mean over the images that show it (both models)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]), precision=precision_of(args), seed=seed,
                       output_bias=utils.bias_from_mean((X * seen).sum(0) / np.maximum(seen.sum(0), 1.0)))
    opt = Adam(args.lr, epsilon=1e-4)
    filled = np.where(mask != 0, X, np.float32(0.0)).astype(np.float32)
    rng = np.random.default_rng(seed)
    trace = []
    for _ in range(args.steps):
        idx = rng.choice(X.shape[0], size=min(args.batch_size, X.shape[0]), replace=False)
        if masked:
            res = model.train_step(X[idx], args.n_samples, 1.0, opt, objective=args.objective, mask=mask[idx])
        else:
            res = model.train_step(filled[idx], args.n_samples, 1.0, opt, objective=args.objective)
        trace.append(float(res[args.objective]))
    return model, trace


def train_resident(args, gray, mask, masked, seed=123):
    """train() through the resident pipeline: gray uint8 [n, 784] in HBM, a new order and binarisation per epoch; masked: the masks resident
    beside the images (the masked step), else the holes filled with grey level 0 and no mask.  Returns (model, the objective per step)."""
    seen = (mask != 0).astype(np.float64)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]), precision=precision_of(args), seed=seed,
                       output_bias=utils.bias_from_mean((gray / 255.0 * seen).sum(0) / np.maximum(seen.sum(0), 1.0)))
    opt = Adam(args.lr, epsilon=1e-4)
    if masked:
        model.set_dataset(gray, mask)
    else:
        model.set_dataset(gray * (mask != 0).astype(np.uint8))
    n = gray.shape[0]
    B = min(args.batch_size, n)
    per_epoch = n // B
    rng = np.random.default_rng(seed)
    trace = []
    for step in range(args.steps):
        if step % per_epoch == 0:
            model.begin_epoch(step // per_epoch, rng.permutation(n).astype(np.int32))
        res = model.train_step_dataset((step % per_epoch) * B, B, args.n_samples, 1.0, opt, objective=args.objective)
        trace.append(float(res[args.objective]))
    return model, trace


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.stochastic_layers != 1:
        raise NotImplementedError("the masked train step covers the 1-layer model only")
    if resident_of(args):
        return main_resident(args)
    X, Xt = load_images(args.images, args.test_images)
    mask = utils.mcar_mask(X.shape, args.rate, seed=args.mask_seed)
    tmask = utils.mcar_mask(Xt.shape, args.rate, seed=args.mask_seed + 1)
    hidden = tmask == 0
    print("images {0}  test images {1}  rate {2:.2f}  steps {3}  draws {4}  precision {5}".format(X.shape[0], Xt.shape[0], args.rate, args.steps, args.draws, precision_of(args)))
    out = {}
    for name, masked in (("masked", True), ("zero_filled", False)):
        model, trace = train(args, X, mask, masked)
        r = model.impute(Xt, tmask, n_samples=args.draws)
        ce, mae = scores(Xt, r["xhat_raw"], hidden) if hidden.any() else (float("nan"), float("nan"))
        out[name] = {"trace": trace, "log_px": float(np.mean(r["log_px"])), "cross_entropy": ce, "abs_error": mae}
        print("{0:<12s} {1} first {2:.4f} last {3:.4f}  log_px_obs {4:.6f}  cross-entropy {5:.6f}  abs error {6:.6f}".format(
            name, args.objective, trace[0], trace[-1], out[name]["log_px"], ce, mae))
    return out


def main_resident(args):
    """main() with both models trained from the resident grey-level set (--resident); the held-out images keep their one fixed binarisation."""
    tr, _ = load_gray(args.images, args.test_images)
    gray = np.clip(np.rint(tr * 255.0), 0, 255).astype(np.uint8)
    _, Xt = load_images(args.images, args.test_images)
    mask = utils.mcar_mask(gray.shape, args.rate, seed=args.mask_seed)
    tmask = utils.mcar_mask(Xt.shape, args.rate, seed=args.mask_seed + 1)
    hidden = tmask == 0
    print("resident  images {0}  test images {1}  rate {2:.2f}  steps {3}  draws {4}  precision {5}".format(gray.shape[0], Xt.shape[0], args.rate, args.steps, args.draws, precision_of(args)))
    out = {}
    for name, masked in (("masked", True), ("zero_filled", False)):
        model, trace = train_resident(args, gray, mask, masked)
        r = model.impute(Xt, tmask, n_samples=args.draws)
        ce, mae = scores(Xt, r["xhat_raw"], hidden) if hidden.any() else (float("nan"), float("nan"))
        out[name] = {"trace": trace, "log_px": float(np.mean(r["log_px"])), "cross_entropy": ce, "abs_error": mae}
        print("{0:<12s} {1} first {2:.4f} last {3:.4f}  log_px_obs {4:.6f}  cross-entropy {5:.6f}  abs error {6:.6f}".format(
            name, args.objective, trace[0], trace[-1], out[name]["log_px"], ce, mae))
    return out


if __name__ == "__main__":
    main()
