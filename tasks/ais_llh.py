"""Annealed importance sampling log p(x) of a 1-layer model main.py trained (Neal 2001; Wu, Burda, Salakhutdinov & Grosse 2017), beside the
k = 5000 importance-weighted bound of main.py:170-184 on the same images, and the bidirectional Monte Carlo gap on data simulated from the
model (Grosse et al. 2015).  Same flags as main.py, plus --weights (the final_weights.npz main.py saved, default
/tmp/iwae/main_<objective>_<layers>_<n_samples>/), --images (test images, the first ones of the fixed binarisation), --chains, --temps,
--leapfrog, --step, --no-adapt, --init and --bdmc (simulated images; 0: skip); with --missing-rate R [--mask-seed S] the images are
incomplete (MCAR masks, utils.device_mcar_mask), every number is of log p(x_obs) and the k = 5000 bound beside the AIS number is iwae_impute's.  The AIS number is a stochastic lower bound that tightens
with --temps; the difference to the k = 5000 number is how much of a reported likelihood is the bound and how much the model.

    python main.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
    python tasks/ais_llh.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo --images 1000
"""
import argparse

import numpy as np

import _common  # noqa: F401  (the repository root on sys.path)

import main as main_mod
import active_units
from iwae_amd import iwae1, utils


def make_parser():
    """main.py's flags (read from main.parser, which stays untouched) plus the sampler's."""
    p = argparse.ArgumentParser(parents=[main_mod.parser], add_help=False)
    p.add_argument("--weights", type=str, default=None,
                   help="final_weights.npz saved by main.py (default: /tmp/iwae/main_<objective>_<layers>_<n_samples>/final_weights.npz)")
    p.add_argument("--images", type=int, default=1000, help="test images")
    p.add_argument("--chains", type=int, default=16, help="chains per image")
    p.add_argument("--temps", type=int, default=1000, help="temperatures (transitions)")
    p.add_argument("--leapfrog", type=int, default=10, help="leapfrog steps per transition")
    p.add_argument("--step", type=float, default=0.1, help="initial HMC step size")
    p.add_argument("--no-adapt", action="store_true", help="fixed step size (the exact scheme)")
    p.add_argument("--init", type=str, default="encoder", choices=("encoder", "prior"), help="base density of the annealing path")
    p.add_argument("--bdmc", type=int, default=16, help="simulated images of the bidirectional check (0: skip)")
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
        raise NotImplementedError("annealed importance sampling covers the 1-layer model only")
    weights = args.weights or active_units.default_weights(args)
    model = iwae1.IWAE(200, 100, device=int(str(args.gpu).split(",")[0]))
    model.load_weights(weights)
    X = active_units.load_test_set()[:args.images]
    kw = dict(n_chains=args.chains, n_temps=args.temps, leapfrog=args.leapfrog, step_size=args.step, adapt=not args.no_adapt, init=args.init)
    mask = mask_of(args, X.shape[0])
    ais, res = model.ais_log_likelihood(X, mask=mask, **kw)
    if mask is None:
        bound, per = model._net.eval_llh(X, k=5000, per_image=True)
    else:       # the same k-sample bound on log p(x_obs): iwae_impute on the same images and mask
        per = model._net.impute(X, mask=mask, n_samples=5000, outputs=("log_px",))["log_px"]
        bound = float(np.mean(per))
        print("missing_rate {0}  mask_seed {1}  observed {2:.4f}".format(args.missing_rate, getattr(args, "mask_seed", 0), float(mask.mean())))
    print("images {0}  chains {1}  temperatures {2}  leapfrog {3}".format(X.shape[0], args.chains, args.temps, args.leapfrog))
    print("ais_log_px {0:.6f}  {3}_k5000 {1:.6f}  difference {2:.6f}".format(ais, bound, ais - bound, "eval_llh" if mask is None else "impute"))
    print("accept_rate {0:.4f}  mean_step {1:.5f}  mean_ess {2:.2f}".format(float(res["accept_rate"].mean()), float(res["step_size"].mean()),
                                                                           float(res["ess"].mean())))
    out = {"ais": ais, "eval_llh": bound, "per_image_ais": res["log_px"], "per_image_eval": per}
    if args.bdmc > 0:
        b = model.bdmc(args.bdmc, mask=mask_of(args, args.bdmc), **kw)
        print("bdmc images {0}  lower {1:.6f}  upper {2:.6f}  gap {3:.6f}".format(args.bdmc, float(b["lower"].mean()), float(b["upper"].mean()), b["gap"]))
        out["bdmc"] = b
    return out


if __name__ == "__main__":
    main()
