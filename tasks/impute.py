"""Missing-pixel imputation with a 1-layer model main.py trained (Mattei & Frellsen 2019, MIWAE): the test images are masked completely
at random at a few rates; per rate the mean k-draw bound on log p(x_obs), the mean ESS/k of the importance weights, and -- on the
UNOBSERVED pixels only -- the Bernoulli cross-entropy and the mean absolute error of the self-normalised importance-sampling estimate
xhat = sum_s al_s sigmoid(l_s), beside two baselines computed on the host: the training set's pixel means, and the decoder's mean at
z = mu(x_in), the encoder's head of the masked input (no sampling, no weights).  Same flags as main.py, plus --weights (the
final_weights.npz main.py saved, default /tmp/iwae/main_<objective>_<layers>_<n_samples>/), --images, --draws, --rates, --mask-seed.

    python main.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
    python tasks/impute.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo --images 1000 --rates 0.25 0.5 0.75
"""
import argparse

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
import active_units
from iwae_amd import iwae1, utils


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the masks' and the estimator's."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    p.add_argument("--images", type=int, default=1000, help="test images")
    p.add_argument("--draws", type=int, default=50, help="importance draws per image (1..65536)")
    p.add_argument("--rates", type=float, nargs="+", default=[0.25, 0.5, 0.75], help="fractions of the pixels hidden, completely at random")
    p.add_argument("--mask-seed", type=int, default=0, help="seed of the masks")
    return p


def train_pixel_means():
    """Per-pixel mean of the training images as run_training loads them (local MNIST or the synthetic stand-in)."""
    data = utils.load_mnist()
    if data is not None:
        Xtrain = data[0][0]
        return np.mean(Xtrain.reshape(Xtrain.shape[0], -1) / 255, axis=0)
    return np.mean(utils.synthetic_mnist()[0], axis=0)


def scores(x, p, hidden):
    """Bernoulli cross-entropy (nats per pixel) and mean absolute error of the probabilities p against x over the `hidden` pixels."""
    x, p = np.asarray(x, dtype=np.float64)[hidden], np.clip(np.asarray(p, dtype=np.float64)[hidden], 1e-7, 1.0 - 1e-7)
    return float(np.mean(-(x * np.log(p) + (1.0 - x) * np.log1p(-p)))), float(np.mean(np.abs(x - p)))


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.stochastic_layers != 1:
        raise NotImplementedError("imputation covers the 1-layer model only")
    weights = args.weights or active_units.default_weights(args)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]))
    model.load_weights(weights)
    X = active_units.load_test_set()[:args.images]
    means = np.broadcast_to(train_pixel_means()[None], X.shape)
    print("images {0}  draws {1}".format(X.shape[0], args.draws))
    out = {}
    for i, rate in enumerate(args.rates):
        mask = utils.mcar_mask(X.shape, rate, seed=args.mask_seed + i)
        hidden = mask == 0
        r = model._net.impute(X, mask=mask, n_samples=args.draws, outputs=("log_px", "xhat", "ess", "q_mu"))
        at_mu = model._net.decode(r["q_mu"])
        row = {"log_px": float(r["log_px"].mean()), "ess_frac": float(np.mean(r["ess"]) / args.draws), "snis": scores(X, r["xhat"], hidden),
               "pixel_means": scores(X, means, hidden), "decoder_at_mu": scores(X, at_mu, hidden)}
        out[rate] = row
        print("rate {0:.2f}  log_px_obs {1:.6f}  ess/k {2:.4f}".format(rate, row["log_px"], row["ess_frac"]))
        for name in ("snis", "pixel_means", "decoder_at_mu"):
            print("    {0:<14s} cross-entropy {1:.6f}  abs error {2:.6f}".format(name, *row[name]))
    return out


if __name__ == "__main__":
    main()
