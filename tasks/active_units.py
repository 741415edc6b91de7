"""Active units of a model main.py trained (Burda et al. section 5.2, Table 1; the reference's README TODO "Investigate active units").
Same flags as main.py, plus --weights: the final_weights.npz main.py saved (default /tmp/iwae/main_<objective>_<layers>_<n_samples>/).
Builds the matching model (1 layer: 200 hidden, 100 latent; 2 layers: [200, 100] hidden, [100, 50] latent), loads the weights, binarises
the test set once with a fixed seed and prints, per stochastic layer, how many units have A_u = Cov_x(E_q[u|x]) > 1e-2.  The
activities, data means and per-image posterior means go to activity.npz next to the weights.

    python main.py --stochastic_layers 2 --n_samples 5 --objective iwae_elbo
    python tasks/active_units.py --stochastic_layers 2 --n_samples 5 --objective iwae_elbo
"""
import argparse
import os

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
from iwae_amd import iwae1, iwae2, utils

THRESHOLD = 1e-2          # Burda et al. section 5.2
N_SAMPLES = 5000          # z1 draws per image for the second layer's E_q[z2|x]
BINARIZE_SEED = 123


def default_weights(args):
    return "/tmp/iwae/main_{0}_{1}_{2}/final_weights.npz".format(args.objective, args.stochastic_layers, args.n_samples)


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus --weights."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    return p


def load_test_set():
    """The test images as run_training loads them (local MNIST or the synthetic stand-in), binarised once with a fixed seed."""
    data = utils.load_mnist()
    if data is not None:
        (_, _), (Xtest, _) = data
        Xtest = Xtest.reshape(Xtest.shape[0], -1) / 255
    else:
        print("NOTE: no local mnist.npz found (set IWAE_MNIST_PATH); using synthetic MNIST-like data")
        _, Xtest = utils.synthetic_mnist()
    rng = np.random.RandomState(BINARIZE_SEED)
    return (rng.random_sample(Xtest.shape) < Xtest).astype(np.float32)


def main(argv=None):
    args = make_parser().parse_args(argv)
    weights = args.weights or default_weights(args)
    device = int(str(args.gpu).split(",")[0])
    if args.stochastic_layers == 1:
        model = iwae1.IWAE(200, 100, device=device)
    else:
        model = iwae2.IWAE([200, 100], [100, 50], device=device)
    model.load_weights(weights)
    Xtest = load_test_set()
    k = N_SAMPLES
    res = model._net.latent_activity(Xtest, k=k, per_image=True)
    counts = [utils.count_active(a, THRESHOLD) for a in res["activity"]]
    for l, (c, a) in enumerate(zip(counts, res["activity"])):
        print("Active units, layer {0}: {1} / {2}".format(l + 1, c, a.size))
    out = {}
    for l in range(len(counts)):
        out["activity_%d" % (l + 1)] = res["activity"][l]
        out["data_mean_%d" % (l + 1)] = res["data_mean"][l]
        out["post_mean_%d" % (l + 1)] = res["post_mean"][l]
    out["counts"] = np.asarray(counts, dtype=np.int64)
    out["threshold"] = np.float64(THRESHOLD)
    out["n_samples"] = np.int64(k)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(weights)), "activity.npz"), **out)
    return counts, res["activity"]


if __name__ == "__main__":
    main()
