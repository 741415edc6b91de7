"""The inference gap of a 1-layer model main.py trained, split as Cremer, Li & Duvenaud (2018, "Inference Suboptimality in Variational
Autoencoders") split it: log p(x) - ELBO[q_enc] = approximation gap (log p(x) - ELBO[q*], q* the best factorised Gaussian of that image)
+ amortisation gap (ELBO[q*] - ELBO[q_enc], what the encoder network loses against q*).  log p(x) comes from annealed importance sampling,
q* from per-image Adam iterations on (mu, log sigma) started at the encoder's heads.  Same flags as main.py, plus --weights (the
final_weights.npz main.py saved, default /tmp/iwae/main_<objective>_<layers>_<n_samples>/), --images, --draws (per image and pass), --iters,
--eval-passes, --local-lr, and the sampler's --chains, --temps, --leapfrog, --step; with --missing-rate R [--mask-seed S] the images are
incomplete (MCAR masks, utils.device_mcar_mask), all three runs take the mask (the split is of log p(x_obs) -
ELBO[q_enc(z | x_obs)]) and iwae_impute's k = 5000 bound on log p(x_obs) is printed beside it.

    python main.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
    python tasks/inference_gaps.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo --images 1000
"""
import argparse

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
import active_units
from iwae_amd import iwae1, utils


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the optimiser's and the sampler's."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    p.add_argument("--images", type=int, default=1000, help="test images")
    p.add_argument("--draws", type=int, default=16, help="draws per image and pass (1..64)")
    p.add_argument("--iters", type=int, default=500, help="Adam iterations on (mu, log sigma) per image")
    p.add_argument("--eval-passes", type=int, default=64, help="evaluation passes of --draws fresh draws each")
    p.add_argument("--local-lr", type=float, default=0.05, help="Adam learning rate of the per-image iterations")
    p.add_argument("--chains", type=int, default=16, help="AIS chains per image")
    p.add_argument("--temps", type=int, default=1000, help="AIS temperatures (transitions)")
    p.add_argument("--leapfrog", type=int, default=10, help="leapfrog steps per transition")
    p.add_argument("--step", type=float, default=0.1, help="initial HMC step size")
    # (no attribute unless given: the namespace of a run without the flags is what it was before they existed; mask_of reads them)
    p.add_argument("--missing-rate", type=float, default=argparse.SUPPRESS,
                   help="score incomplete images: this fraction of the pixels hidden completely at random (utils.device_mcar_mask, the masks "
                        "tasks/miwae.py --resident trains under)")
    p.add_argument("--mask-seed", type=int, default=argparse.SUPPRESS, help="seed of the masks (default 0)")
    return p


def mask_of(args, n, x_dim=784):
    """The [n, x_dim] mask of --missing-rate / --mask-seed (uint8, 1 = observed), or None without --missing-rate."""
    if not hasattr(args, "missing_rate"):
        return None
    return utils.device_mcar_mask(n, x_dim, args.missing_rate, seed=getattr(args, "mask_seed", 0))


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.stochastic_layers != 1:
        raise NotImplementedError("the inference-gap split covers the 1-layer model only")
    weights = args.weights or active_units.default_weights(args)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]))
    model.load_weights(weights)
    X = active_units.load_test_set()[:args.images]
    mask = mask_of(args, X.shape[0])
    g = model.inference_gaps(X, mask=mask, n_samples=args.draws, n_iters=args.iters, n_eval=args.eval_passes, lr=args.local_lr,
                             ais=dict(n_chains=args.chains, n_temps=args.temps, leapfrog=args.leapfrog, step_size=args.step))
    print("images {0}  draws {1}  iterations {2}  evaluation passes {3}".format(X.shape[0], args.draws, args.iters, args.eval_passes))
    print("log_px {0:.6f}  elbo_amortized {1:.6f}  elbo_local {2:.6f}".format(float(g["log_px"].mean()), float(g["elbo_amortized"].mean()),
                                                                            float(g["elbo_local"].mean())))
    print("approximation_gap {0:.6f}  amortization_gap {1:.6f}  inference_gap {2:.6f}".format(
        float(g["approximation_gap"].mean()), float(g["amortization_gap"].mean()), float(np.mean(g["log_px"] - g["elbo_amortized"]))))
    if mask is not None:
        g["impute_log_px"] = model._net.impute(X, mask=mask, n_samples=5000, outputs=("log_px",))["log_px"]
        print("missing_rate {0}  mask_seed {1}  observed {2:.4f}  impute_k5000 {3:.6f}  ais_minus_impute {4:.6f}".format(
            args.missing_rate, getattr(args, "mask_seed", 0), float(mask.mean()), float(g["impute_log_px"].mean()),
            float(np.mean(g["log_px"] - g["impute_log_px"]))))
    return g


if __name__ == "__main__":
    main()
