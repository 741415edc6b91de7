"""Aggregate-posterior decomposition of the KL term of a 1-layer model main.py trained (Hoffman & Johnson 2016, "ELBO surgery"; Chen et al.
2018, beta-TCVAE).  Same flags as main.py, plus --weights (the final_weights.npz main.py saved, default
/tmp/iwae/main_<objective>_<layers>_<n_samples>/) and --draws (samples of q(z|x) per image).  Builds the 1-layer model (200 hidden, 100
latent), loads the weights, binarises the test set once with a fixed seed and prints the four scalars of
mean_n KL(q(z|x_n) || p(z)) = mi + tc + dim_kl, log N, and one line per latent unit: the activity A_u of tasks/active_units.py beside
unit_kl = KL(q(z_d) || p(z_d)) and unit_mi = I(n; z_d).  A collapsed unit has all three near 0.

    python main.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
    python tasks/elbo_surgery.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
"""
import argparse

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
import active_units
from iwae_amd import iwae1


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus --weights and --draws."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    p.add_argument("--draws", type=int, default=1, help="samples of q(z|x) per test image")
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.stochastic_layers != 1:
        raise NotImplementedError("the aggregate posterior covers the 1-layer model only")
    weights = args.weights or active_units.default_weights(args)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]))
    model.load_weights(weights)
    Xtest = active_units.load_test_set()
    _, act = model.active_units(Xtest)
    res = model.aggregate_posterior(Xtest, n_samples=args.draws)
    print("images {0}  draws {1}  log N {2:.12g}".format(Xtest.shape[0], args.draws, res["log_n"]))
    for key in ("kl", "mi", "tc", "dim_kl"):
        print("{0} {1:.12g}".format(key, res[key]))
    for d in range(res["unit_kl"].size):
        print("unit {0:3d}  A_u {1:.6e}  unit_kl {2:.12e}  unit_mi {3:.12e}".format(d, act[0][d], res["unit_kl"][d], res["unit_mi"][d]))
    return res, act[0]


if __name__ == "__main__":
    main()
