"""The posterior p(z | x) in latent space of a 1-layer model main.py trained, by the two uses of the self-normalised importance weights the
reference's README names: the SNIS estimate of its mean and covariance, and sampling importance resampling (tasks/task01.py does both
on the host, one image at a time).  Per image: the ratio of the posterior's variance to q's per latent unit (below 1: the encoder's q is
too wide there; above 1: too narrow) and the largest |correlation| between two units, which no factorised Gaussian can represent -- the
approximation gap of Cremer et al. 2018.  The resampled draws and the moments are saved to an .npz.  Same flags as main.py, plus
--weights (the final_weights.npz main.py saved, default /tmp/iwae/main_<objective>_<layers>_<n_samples>/), --images, --draws,
--resamples, --rate (fraction of the pixels hidden completely at random; 0: none), --mask-seed, --out.

    python main.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
    python tasks/posterior.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo --images 100 --draws 5000 --resamples 200
"""
import argparse
import os

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
import active_units
from iwae_amd import iwae1, utils


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the estimator's."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    p.add_argument("--images", type=int, default=100, help="test images")
    p.add_argument("--draws", type=int, default=5000, help="importance draws per image (1..65536)")
    p.add_argument("--resamples", type=int, default=200, help="latent vectors resampled per image (0..65536)")
    p.add_argument("--rate", type=float, default=0.0, help="fraction of the pixels hidden, completely at random (0: every pixel observed)")
    p.add_argument("--mask-seed", type=int, default=0, help="seed of the mask")
    p.add_argument("--out", type=str, default=None, help="the .npz to write (default: posterior.npz beside the weights)")
    return p


def summary(cov, q_sigma):
    """Per image: the posterior / q variance ratio per unit [N, D] and the largest |correlation| between two units [N]."""
    cov = np.asarray(cov, dtype=np.float64)
    var = np.diagonal(cov, axis1=1, axis2=2)
    ratio = var / np.asarray(q_sigma, dtype=np.float64) ** 2
    sd = np.sqrt(np.maximum(var, 1e-300))
    corr = cov / (sd[:, :, None] * sd[:, None, :])
    corr[:, np.arange(cov.shape[1]), np.arange(cov.shape[1])] = 0.0
    return ratio, np.max(np.abs(corr), axis=(1, 2))


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.stochastic_layers != 1:
        raise NotImplementedError("the latent posterior covers the 1-layer model only")
    weights = args.weights or active_units.default_weights(args)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]))
    model.load_weights(weights)
    X = active_units.load_test_set()[:args.images]
    mask = utils.mcar_mask(X.shape, args.rate, seed=args.mask_seed) if args.rate > 0 else None
    r = model.posterior(X, mask=mask, n_samples=args.draws, n_draws=args.resamples)
    ratio, corr = summary(r["cov"], r["q_sigma"])
    print("images {0}  draws {1}  resamples {2}  log_px {3:.6f}  ess/k {4:.4f}".format(X.shape[0], args.draws, args.resamples, float(r["log_px"].mean()),
                                                                              float(np.mean(r["ess"]) / args.draws)))
    for n in range(X.shape[0]):
        print("image {0:4d}  variance ratio min {1:.4f} median {2:.4f} max {3:.4f}  largest |correlation| {4:.4f}".format(
            n, float(ratio[n].min()), float(np.median(ratio[n])), float(ratio[n].max()), float(corr[n])))
    out = args.out or os.path.join(os.path.dirname(weights), "posterior.npz")
    keep = {key: r[key] for key in ("log_px", "ess", "mean", "cov", "q_mu", "q_sigma") if key in r}
    if args.resamples > 0:
        keep.update(idx=r["idx"], z=r["z"])
    np.savez(out, variance_ratio=ratio, max_abs_correlation=corr, **keep)
    print("saved {0}".format(out))
    return {"variance_ratio": ratio, "max_abs_correlation": corr, "out": out}


if __name__ == "__main__":
    main()
