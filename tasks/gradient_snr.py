"""Signal-to-noise ratio of the training gradient estimator against k (the property behind tasks/task02.py; Rainforth et al. 2018,
arXiv 1802.04537; Tucker et al. 2019, arXiv 1810.04152).  Same flags as main.py, plus --weights, --k_list, --draws and --estimator
(default: --objective; also `dreg`, the 1-layer model only).  Builds the matching model, loads the weights (default: the
final_weights.npz main.py saved, or tasks/task02.py's for dreg), takes the first --batch_size test images binarised as
tasks/active_units.py binarises them and, for every k, draws the gradient --draws times (iwae_grad_moments).  Prints one line per k
with the encoder's and the decoder's SNR (the mean over parameters of |mean| / sd) and summed variance; the summaries and the
per-parameter moments go to gradient_snr.npz next to the weights.

    python main.py --n_samples 5 --objective iwae_elbo
    python tasks/gradient_snr.py --n_samples 5 --objective iwae_elbo --k_list 1,5,50,500
"""
import argparse
import os

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import active_units
import main as main_mod
from iwae_amd import iwae1, iwae2

K_LIST = "1,5,50,500,5000"
DRAWS = 1000
GROUPS = ("encoder", "decoder")
STATS = ("snr", "variance", "signal")


def default_weights(args):
    if estimator(args) == "dreg":
        return "/tmp/iwae/task02_{0}/final_weights.npz".format(args.n_samples)
    return "/tmp/iwae/main_{0}_{1}_{2}/final_weights.npz".format(args.objective, args.stochastic_layers, args.n_samples)


def estimator(args):
    return args.estimator or args.objective


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the four of this driver."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz to load (default: main.py's /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz, "
                        "for dreg tasks/task02.py's /tmp/iwae/task02_<n_samples>/final_weights.npz)")
    p.add_argument("--k_list", type=str, default=K_LIST, help="comma-separated numbers of importance samples")
    p.add_argument("--draws", type=int, default=DRAWS, help="gradient draws per k (>= 2)")
    p.add_argument("--estimator", type=str, default=None, choices=["vae_elbo", "iwae_elbo", "iwae_eq14", "vae_elbo_kl", "dreg"],
                   help="the gradient estimator (default: --objective); dreg: tasks/task02.py's, 1 layer only")
    return p


def parse_args(argv=None):
    p = make_parser()
    args = p.parse_args(argv)
    if args.stochastic_layers == 2 and estimator(args) in ("dreg", "vae_elbo_kl"):
        p.error("--estimator %s is defined for the 1-layer model only" % estimator(args))
    try:
        args.k_values = [int(v) for v in args.k_list.split(",") if v.strip()]
    except ValueError:
        p.error("--k_list: comma-separated integers, got %r" % args.k_list)
    if not args.k_values or min(args.k_values) < 1:
        p.error("--k_list: need at least one k, every k >= 1")
    if args.draws < 2:
        p.error("--draws must be >= 2")
    return args


def main(argv=None):
    args = parse_args(argv)
    weights = args.weights or default_weights(args)
    est = estimator(args)
    device = int(str(args.gpu).split(",")[0])
    if args.stochastic_layers == 1:
        model = iwae1.IWAE(200, 100, device=device)
    else:
        model = iwae2.IWAE([200, 100], [100, 50], device=device)
    model.load_weights(weights)
    x = active_units.load_test_set()[:args.batch_size]
    model._net.set_step(0)
    out = {"k": np.asarray(args.k_values, dtype=np.int64), "draws": np.int64(args.draws), "batch_size": np.int64(x.shape[0]),
           "estimator": np.array(est)}
    rows = {"%s_%s" % (g, s): [] for g in GROUPS for s in STATS}
    print("gradient SNR of {0} at B = {1}, {2} draws per k ({3})".format(est, x.shape[0], args.draws, weights))
    for k in args.k_values:
        r = model.gradient_snr(x, k, n_draws=args.draws, objective=est)
        for g in GROUPS:
            for s in STATS:
                rows["%s_%s" % (g, s)].append(r[g][s])
        out["mean_k%d" % k], out["var_k%d" % k] = r["mean"], r["var"]
        print("k = {0:5d}: encoder SNR {1:.4g} variance {2:.4g} | decoder SNR {3:.4g} variance {4:.4g}".format(
            k, r["encoder"]["snr"], r["encoder"]["variance"], r["decoder"]["snr"], r["decoder"]["variance"]))
    for key, v in rows.items():
        out[key] = np.asarray(v, dtype=np.float64)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(weights)), "gradient_snr.npz"), **out)
    return rows


if __name__ == "__main__":
    main()
