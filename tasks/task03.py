"""Driver of the reference's tasks/task03.py: the 2-layer IWAE with a 2-D top latent ([200, 100] hidden, [4, 2] latent, tasks/task03.py:84-86),
same flags (no --stochastic_layers), main.py's loop (run_training).  Plots are out of scope; the grid quadrature of
tasks/task01.py covers the 1-layer model only (the 2-layer model needs a nested integral over z1).

    python tasks/task03.py --n_samples 50 --objective vae_elbo
"""
from _common import parser_task03

from iwae_amd import iwae2
from main import run_training


def main(argv=None):
    args = parser_task03().parse_args(argv)
    string = "task03_{0}_{1}_{2}".format(args.objective, 2, args.n_samples)      # tasks/task03.py:31
    if args.objective == "vae_elbo_kl":
        raise KeyError(args.objective)          # src/iwae2.py:154-167
    return run_training(args, string, lambda **kw: iwae2.IWAE([200, 100], [4, 2], **kw), args.objective)


if __name__ == "__main__":
    main()
