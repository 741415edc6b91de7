"""Reference API of src/iwae2.py (two stochastic layers, src/iwae2.py:99-182)."""
import numpy as np

from . import utils
from ._shim import BaseIWAE, _Sub, as_tensor


class IWAE(BaseIWAE):
    n_layers = 2
    scalar_keys = ("vae_elbo", "iwae_elbo", "iwae_eq14")    # src/iwae2.py:154-156 (no vae_elbo_kl: KeyError)

    def __init__(self, n_hidden, n_latent, **kwargs):
        super().__init__([int(v) for v in n_hidden], [int(v) for v in n_latent], **kwargs)
        self.encoder = _Sub(self, 0, 16)     # encode_x_to_z1, encode_z1_to_z2   src/iwae2.py:55-56
        self.decoder = _Sub(self, 16, 30)    # decode_z2_to_z1, decode_z1_to_x   src/iwae2.py:77-87

    def val_step(self, x, n_samples, beta, outputs=None, mask=None):
        return self.call(x, n_samples, beta, outputs=outputs, mask=mask)

    def _check_mask(self, mask):
        raise ValueError("the masked step covers the 1-layer model only: the 2-layer encoder q(z2|z1) q(z1|x) has no masked form here")

    def sample(self, z2):
        """src/iwae2.py:184-196: z1 ~ p(z1|z2), probs = sigmoid(decoder(z1)), x_sample ~ Bernoulli(probs)."""
        probs = self._net.decode(np.asarray(z2, dtype=np.float32))
        x_sample = (np.random.random_sample(probs.shape) < probs).astype(np.float32)
        return as_tensor(x_sample), as_tensor(probs)

    def true_posterior(self, x, z_grid, log_wq=None):
        raise NotImplementedError("the grid posterior covers the 1-layer model only: p(x) of the 2-layer model needs a nested integral over z1 "
                                  "for every z2 of the grid")

    def true_log_likelihood(self, X, extent=(-5.0, 5.0), n_per_dim=None, batch=10000):
        self.true_posterior(X, None)

    def active_units(self, X, n_samples=5000, threshold=1e-2):
        """Units of each stochastic layer with A_u = Cov_x(E_q[u|x]) > threshold over the images X: E_q[z1|x] = mu1(x),
        E_q[z2|x] = the mean of mu2(z1) over n_samples draws of z1 ~ q(z1|x).  Returns ([count z1, count z2], [A z1, A z2])."""
        act = self._net.latent_activity(np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim), k=n_samples)["activity"]
        return [utils.count_active(a, threshold) for a in act], act

    def aggregate_posterior(self, X, n_samples=1):
        raise NotImplementedError("the aggregate posterior covers the 1-layer model only: q(z2|x) of the 2-layer model is not Gaussian and "
                                  "its p(z1) is not N(0,1)")

    def ais_log_likelihood(self, X, mask=None, n_chains=16, n_temps=1000, **kwargs):
        raise NotImplementedError("annealed importance sampling covers the 1-layer model only: the 2-layer chain would have to move (z1, z2) "
                                  "jointly under p(z1|z2) p(z2)")

    def bdmc(self, n, n_chains=16, n_temps=1000, seed=0, **kwargs):
        self.ais_log_likelihood(None)

    def local_posterior(self, X, mask=None, n_samples=16, n_iters=200, n_eval=8, **kwargs):
        raise NotImplementedError("per-image posterior optimisation covers the 1-layer model only: the 2-layer q(z2|z1) q(z1|x) is not one "
                                  "factorised Gaussian per image")

    def inference_gaps(self, X, **kwargs):
        self.local_posterior(None)

    def impute(self, X, mask, n_samples=50, **kwargs):
        raise ValueError("imputation covers the 1-layer model only: the 2-layer proposal q(z2|z1) q(z1|x) needs its own weights")

    def reconstruct(self, X, n_samples=50, **kwargs):
        self.impute(None, None)

    def posterior(self, X, mask=None, n_samples=5000, n_draws=0, **kwargs):
        raise ValueError("the latent posterior covers the 1-layer model only: the 2-layer proposal q(z2|z1) q(z1|x) needs its own weights")

    def multiple_imputations(self, X, mask, n_samples=5000, n_draws=5, seed=0, **kwargs):
        self.posterior(None)
