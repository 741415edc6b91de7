"""Driver of the reference's tasks/task01.py: the IWAE with a 2-D latent space (hidden 200, latent 2 for one stochastic layer; [200, 100] and
[2, 2] for two, tasks/task01.py:83-90), same flags, main.py's loop (run_training).  After the k = 5000 test-set estimate, the 1-layer model
also gets what tasks/plot_task01.py:31-88 computes, without the plots:

  * the test-set log p(x) by quadrature on one shared latent grid (IWAE.true_log_likelihood) -- the ground truth the k = 5000 bound sits
    just below;
  * for the first N_EXAMPLES test images, the true and the variational posterior on a POST_GRID x POST_GRID grid around q(z|x)
    (q_mu +- 2 q_std, clipped to [-3, 3], plot_task01.py:44-55) and the sampling-importance-resampling draws of a k = SIR_K forward
    (plot_task01.py:74-88), saved to /tmp/iwae/<string>/posteriors.npz.

    python tasks/task01.py --stochastic_layers 1 --n_samples 5 --objective iwae_elbo
"""
import os

import numpy as np

from _common import parser_task01

from iwae_amd import iwae1, iwae2
from main import run_training

N_EXAMPLES = 20          # plot_task01.py:196
POST_GRID = 200          # plot_task01.py:45-46 (n1 = n2)
SIR_K = 10000            # plot_task01.py:197 (L)
SIR_DRAWS = 200          # plot_task01.py:76
LLH_GRID = None          # points per dimension of true_log_likelihood's shared grid (None: its default)


def posterior_panels(model, X, n_examples=None, n_grid=None, sir_k=None, sir_draws=None):
    """plot_task01.py:31-88 without matplotlib: per image its own grid around q(z|x) and the arrays drawn there."""
    n_examples = N_EXAMPLES if n_examples is None else n_examples
    n_grid = POST_GRID if n_grid is None else n_grid
    sir_k = SIR_K if sir_k is None else sir_k
    sir_draws = min(SIR_DRAWS if sir_draws is None else sir_draws, sir_k)
    from iwae_amd import utils
    X = np.asarray(X, dtype=np.float32)[:n_examples]
    D = model._net.n_latent[0]
    heads = model._net.grid_posterior(X, np.zeros((1, D), dtype=np.float32))      # (q_mu, q_sigma of every image; the 1-point grid is not used)
    out = {k: [] for k in ("log_posterior", "variational_posterior", "ranges", "log_px", "q_mass", "sir_idx", "z")}
    for i, x in enumerate(X):
        mu, sd = heads["q_mu"][i], heads["q_sigma"][i]
        ranges = [(max(-3.0, mu[d] - 2 * sd[d]), min(3.0, mu[d] + 2 * sd[d])) for d in range(D)]       # plot_task01.py:47-52
        grid, lw = utils.latent_grid(ranges, n_grid)
        # (log_posterior + w: the posterior mass of each cell; with one cell weight for the whole grid that is lj - logsumexp_g(lj), what
        # plot_task01.py:60-63 draws, while log_px and q_mass are the quadrature values)
        tp = model.true_posterior(x[None], grid, lw)
        out["log_posterior"].append((tp["log_posterior"][0] + lw).reshape(n_grid, n_grid).astype(np.float32))
        out["variational_posterior"].append(tp["variational_posterior"][0].reshape(n_grid, n_grid).astype(np.float32))
        out["ranges"].append(np.asarray(ranges, dtype=np.float32))
        out["log_px"].append(tp["log_px"][0])
        out["q_mass"].append(tp["q_mass"][0])
        # ---- sampling importance resampling (plot_task01.py:74-88)
        res = model(x[None], sir_k, outputs=("z", "lpxz", "lpz", "lqzx"))
        log_w = (np.asarray(res["lpxz"]) + np.asarray(res["lpz"]) - np.asarray(res["lqzx"])).reshape(-1).astype(np.float64)
        al = np.exp(log_w - log_w.max())
        al /= al.sum()
        out["sir_idx"].append(np.random.choice(np.arange(sir_k), size=sir_draws, replace=False, p=al))
        out["z"].append(np.asarray(res["z"]).reshape(sir_k, D))
    return {k: np.stack(v) for k, v in out.items()}


def main(argv=None):
    args = parser_task01().parse_args(argv)
    string = "task01_{0}_{1}_{2}".format(args.objective, args.stochastic_layers, args.n_samples)      # tasks/task01.py:30
    held = {}

    def make_model(**kw):
        if args.stochastic_layers == 1:
            model = iwae1.IWAE(200, 2, **kw)
        else:
            model = iwae2.IWAE([200, 100], [2, 2], **kw)
        evaluate = model.eval_llh

        def eval_llh(X, *a, **k):      # the binarised test set run_training evaluates: the quadrature below scores the same images
            held["Xtest"] = X
            return evaluate(X, *a, **k)

        model.eval_llh = eval_llh
        held["model"] = model
        return model

    if args.stochastic_layers == 2 and args.objective == "vae_elbo_kl":
        raise KeyError(args.objective)          # src/iwae2.py:154-167
    llh = run_training(args, string, make_model, args.objective)
    if args.stochastic_layers == 1:
        model, Xtest = held["model"], held["Xtest"]
        grid_llh, _ = model.true_log_likelihood(Xtest, n_per_dim=LLH_GRID)
        print("Test-set grid-quadrature log likelihood: {:.4f}".format(grid_llh))
        panels = posterior_panels(model, Xtest)
        os.makedirs("/tmp/iwae/{0}".format(string), exist_ok=True)
        np.savez("/tmp/iwae/{0}/posteriors.npz".format(string), **panels)
    return llh


if __name__ == "__main__":
    main()
