"""Reference API of src/iwae1.py on the MI355X-native step: IWAE(n_hidden, n_latent),
model(x, n_samples, beta), train_step, val_step, sample (src/iwae1.py:88-178)."""
import numpy as np

from . import utils
from ._shim import BaseIWAE, _Sub, as_tensor
from .native import ais_schedule


class IWAE(BaseIWAE):
    n_layers = 1
    scalar_keys = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")   # src/iwae1.py:141-144

    def __init__(self, n_hidden, n_latent, **kwargs):
        super().__init__(int(n_hidden), int(n_latent), **kwargs)
        self.encoder = _Sub(self, 0, 8)     # l1, l2, lmu, lstd (kernel, bias)   src/iwae1.py:54
        self.decoder = _Sub(self, 8, 14)    # three Dense                        src/iwae1.py:70-77

    def sample(self, z):
        """src/iwae1.py:168-178: (x_sample ~ Bernoulli(probs), probs = sigmoid(decoder(z)))."""
        probs = self._net.decode(np.asarray(z, dtype=np.float32))
        x_sample = (np.random.random_sample(probs.shape) < probs).astype(np.float32)
        return as_tensor(x_sample), as_tensor(probs)

    # ---- ground truth for low-dimensional latents (tasks/plot_task01.py:31-78): quadrature on a latent grid
    def _grid_scope(self):
        if self._net.cond_dim:
            raise NotImplementedError("the grid posterior covers the unconditional 1-layer model only (a conditional model needs the label of "
                                      "every image inside the decoder and the prior)")

    def true_posterior(self, x, z_grid, log_wq=None):
        """True posterior p(z|x) on the points z_grid [G, D] (log quadrature weights log_wq [G], None: 0) -- the arrays
        tasks/plot_task01.py:61-72 draws.  Returns iwae_grid_posterior's dict (log_px, post_mean, post_cov, q_mu, q_sigma, q_mass,
        kl_q_post, log_joint) plus log_posterior = log_joint - log_px, the log density of p(z|x) at the points (normalised: logsumexp
        over the grid of log_posterior + w is 0; log_posterior + w is the posterior mass of each cell, what plot_task01.py:60-63 draws
        on a uniform grid) and variational_posterior = log q(z_g|x) (the encoder's Normal, src/iwae1.py:39-42), both [N, G]."""
        self._grid_scope()
        x = np.asarray(x, dtype=np.float32).reshape(-1, self._net.x_dim)
        z_grid = np.asarray(z_grid, dtype=np.float32)
        res = self._net.grid_posterior(x, z_grid, log_wq, log_joint=True)
        res["log_posterior"] = res["log_joint"].astype(np.float64) - res["log_px"][:, None]
        zg = z_grid.reshape(z_grid.shape[0], -1).astype(np.float64)
        mu, sg = res["q_mu"].astype(np.float64), res["q_sigma"].astype(np.float64)
        u = (zg[None, :, :] - mu[:, None, :]) / sg[:, None, :]
        res["variational_posterior"] = np.sum(-0.5 * u * u - np.log(sg)[:, None, :] - 0.5 * np.log(2 * np.pi), axis=-1)
        return res

    def true_log_likelihood(self, X, extent=(-5.0, 5.0), n_per_dim=None, batch=10000):
        """Test-set log p(x) by quadrature on ONE uniform grid [extent]^D shared by every image (D <= 2; n_per_dim points per dimension,
        default 1000 for D = 2, 20000 for D = 1), the images fed `batch` at a time.  Returns (mean, per_image float64 [N]).  Check the
        grid with true_posterior's q_mass first: near 1 means the grid covers and resolves q(z|x)."""
        self._grid_scope()
        D = self._net.n_latent[0]
        if D > 2:
            raise NotImplementedError("true_log_likelihood: a shared uniform grid is for 1 or 2 latent dimensions (got %d); call "
                                      "true_posterior with a grid of your own" % D)
        n = n_per_dim or (1000 if D == 2 else 20000)
        z, lw = utils.latent_grid([extent] * D, n)
        X = np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim)
        per = np.concatenate([self._net.grid_posterior(X[i:i + batch], z, lw)["log_px"] for i in range(0, X.shape[0], batch)])
        return float(np.mean(per)), per

    # ---- active units (Burda et al. section 5.2; the reference's README TODO)
    def active_units(self, X, threshold=1e-2):
        """Units of the latent layer with A_u = Cov_x(E_q[u|x]) > threshold over the images X (E_q[z|x] = mu(x), the encoder head).
        Returns (counts per layer, activity per layer): ([count], [A float64 [D]])."""
        act = self._net.latent_activity(np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim))["activity"]
        return [utils.count_active(a, threshold) for a in act], act

    # ---- aggregate-posterior decomposition of the KL term (Hoffman & Johnson 2016; Chen et al. 2018)
    def aggregate_posterior(self, X, n_samples=1):
        """mean_n KL(q(z|x_n) || p(z)) over the images X split into mi + tc + dim_kl (iwae_aggregate_posterior), with the per-unit
        unit_kl[d] = KL(q(z_d) || p(z_d)) and unit_mi[d] = I(n; z_d): both near 0 for a collapsed unit.  Returns the binding's dict."""
        if self._net.cond_dim:
            raise NotImplementedError("the aggregate posterior covers the unconditional 1-layer model only (q(z|x, y) and a learned p(z|y) "
                                      "need a label per image)")
        return self._net.aggregate_posterior(np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim), n_samples=n_samples)

    # ---- annealed importance sampling (Neal 2001; Wu et al. 2017) and its check on simulated data (Grosse et al. 2015)
    def _ais_scope(self):
        if self._net.cond_dim:
            raise NotImplementedError("annealed importance sampling covers the unconditional 1-layer model only")

    def ais_log_likelihood(self, X, mask=None, n_chains=16, n_temps=1000, **kwargs):
        """Test-set log p(x) by annealed importance sampling with HMC transitions (iwae_ais): a stochastic lower bound that tightens
        with n_temps where the k-sample bound of the evaluator is limited by the encoder.  mask [N, x_dim] (non-zero = observed): the
        images are incomplete and the estimate is of log p(x_obs) (iwae_ais_masked), the tight counterpart of impute()'s bound; what X
        holds at an unobserved pixel is never read.  Returns (mean, the binding's dict)."""
        self._ais_scope()
        res = self._net.ais(np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim), n_chains=n_chains, n_temps=n_temps, mask=mask, **kwargs)
        return float(np.mean(res["log_px"])), res

    def bdmc(self, n, n_chains=16, n_temps=1000, seed=0, schedule="sigmoid", mask=None, **kwargs):
        """Bidirectional Monte Carlo on n images simulated from the model: z ~ N(0, I), x ~ Bernoulli(decode(z)) (a seeded host generator),
        so z is an exact posterior sample of x.  The forward run (ascending betas) gives a stochastic lower bound of log p(x), the reverse
        run (descending betas, every chain started at the exact sample) a stochastic upper bound, upper = -(LSE_c log_w_rev - log C).
        kwargs (leapfrog, step_size, adapt, init) go to both runs.  mask: an [n, x_dim] array (non-zero = observed) or a callable on the
        simulated x that returns one; both runs then bracket log p(x_obs).  The simulated z is still an exact posterior sample given x_obs
        alone -- x_obs is a marginal of x, so (z, x_obs) is a joint draw of p(z) p(x_obs|z) -- and the reverse run stays valid.
        Returns {"x", "z", "lower", "upper" [n] float64, "gap": mean(upper - lower), "forward", "reverse": the two runs' dicts}, with a mask also "mask"."""
        self._ais_scope()
        rng = np.random.default_rng(seed)
        D = self._net.n_latent[0]
        z = rng.standard_normal((int(n), D)).astype(np.float32)
        probs = self._net.decode(z)
        x = (rng.random(probs.shape) < probs).astype(np.float32)
        betas = ais_schedule(n_temps, schedule)
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask(x) if callable(mask) else mask) != 0, dtype=np.uint8).reshape(x.shape)
            kwargs = dict(kwargs, mask=mask)
        fwd = self._net.ais(x, n_chains=n_chains, betas=betas, **kwargs)
        z0 = np.ascontiguousarray(np.broadcast_to(z[None], (int(n_chains),) + z.shape))
        rev = self._net.ais(x, n_chains=n_chains, betas=betas[::-1].copy(), z0=z0, **kwargs)
        lw = rev["log_w"]
        m = lw.max(axis=0)
        upper = -(m + np.log(np.mean(np.exp(lw - m[None]), axis=0)))
        lower = fwd["log_px"]
        out = {"x": x, "z": z, "lower": lower, "upper": upper, "gap": float(np.mean(upper - lower)), "forward": fwd, "reverse": rev}
        if mask is not None:
            out["mask"] = mask
        return out

    # ---- per-image posterior optimisation and the inference-gap split (Cremer, Li & Duvenaud 2018)
    def _local_scope(self):
        if self._net.cond_dim:
            raise NotImplementedError("per-image posterior optimisation covers the unconditional 1-layer model only")

    def local_posterior(self, X, mask=None, n_samples=16, n_iters=200, n_eval=8, **kwargs):
        """The best factorised Gaussian q*(z|x) of every image of X found by n_iters Adam iterations on (mu, log sigma) from the encoder's
        q(z|x) (iwae_local_posterior; kwargs: objective, lr, start, noise, trace, beta_1, beta_2, epsilon).  mask [N, x_dim] (non-zero =
        observed): q* is fitted to p(z | x_obs) from the encoder's q(z | x_obs) (iwae_local_posterior_masked).  Returns the binding's dict."""
        self._local_scope()
        return self._net.local_posterior(np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim), n_samples=n_samples, n_iters=n_iters,
                                         n_eval=n_eval, mask=mask, **kwargs)

    def inference_gaps(self, X, mask=None, n_samples=16, n_iters=200, n_eval=64, lr=0.05, ais=None):
        """log p(x) - ELBO[q_enc] of every image of X split into the approximation gap log p(x) - ELBO[q*] (what no factorised Gaussian
        can close) and the amortisation gap ELBO[q*] - ELBO[q_enc] (what the encoder loses against the best one).  log p(x): annealed
        importance sampling (ais: the arguments of ais_log_likelihood); ELBO[q_enc]: n_eval passes of n_samples draws from the encoder's
        q (no iterations); ELBO[q*]: the same after n_iters ELBO iterations.  Returns per-image float64 arrays log_px, elbo_amortized,
        elbo_local, approximation_gap, amortization_gap, the standard errors elbo_amortized_se and elbo_local_se of the two means (from the
        evaluation log-weights), log_px_se (delta method over the chains) and the three runs' dicts (ais, amortized, local).  mask
        [N, x_dim] (non-zero = observed): all three runs take it, and the split is of log p(x_obs) - ELBO[q_enc(z | x_obs)]."""
        self._local_scope()
        X = np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim)
        _, a = self.ais_log_likelihood(X, mask=mask, **(ais or {}))
        amort = self._net.local_posterior(X, n_samples=n_samples, n_iters=0, n_eval=n_eval, objective="elbo", mask=mask)
        local = self._net.local_posterior(X, n_samples=n_samples, n_iters=n_iters, n_eval=n_eval, objective="elbo", lr=lr, mask=mask)
        out = utils.inference_gap_split(a["log_px"], amort["elbo"], local["elbo"])
        out["elbo_amortized_se"], out["elbo_local_se"] = utils.mean_se(amort["log_w"]), utils.mean_se(local["log_w"])
        out["log_px_se"] = utils.log_mean_exp_se(a["log_w"])
        out.update(ais=a, amortized=amort, local=local)
        return out

    # ---- missing-pixel imputation and importance-weighted reconstruction (Mattei & Frellsen 2019, MIWAE)
    def impute(self, X, mask, n_samples=50, **kwargs):
        """Given the pixels of X that mask marks as observed (non-zero; None: all of them): the n_samples-draw bound log_px on
        log p(x_obs) per image and the self-normalised importance-sampling estimate of E[x | x_obs] (iwae_impute; kwargs: noise).  Returns
        {"xhat": the estimate with the observed pixels put back exactly as given, "xhat_raw": the estimate at every pixel, "log_px"
        (float64), "ess"} -- what X holds at an unobserved pixel is never read."""
        if self._net.cond_dim:
            raise NotImplementedError("imputation covers the unconditional 1-layer model only")
        X = np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim)
        r = self._net.impute(X, mask=mask, n_samples=n_samples, outputs=("log_px", "xhat", "ess"), **kwargs)
        filled = X.copy() if mask is None else np.where(np.asarray(mask).reshape(X.shape) != 0, X, r["xhat"])
        return {"xhat": filled, "xhat_raw": r["xhat"], "log_px": r["log_px"], "ess": r["ess"]}

    def reconstruct(self, X, n_samples=50, **kwargs):
        """The importance-weighted reconstruction of X: impute() with every pixel observed, whose xhat_raw is sum_s al_s sigmoid(l_s).
        Returns impute()'s dict with "xhat" = that reconstruction."""
        r = self.impute(X, None, n_samples=n_samples, **kwargs)
        r["xhat"] = r["xhat_raw"]
        return r

    # ---- the posterior in latent space: SNIS moments and sampling importance resampling (the reference's README; tasks/task01.py:52-58)
    def posterior(self, X, mask=None, n_samples=5000, n_draws=0, **kwargs):
        """The self-normalised estimates of the mean and covariance of p(z | x_obs) of every image of X, and n_draws latent vectors per
        image resampled from it (iwae_posterior; kwargs: noise, uniforms, outputs).  Returns the binding's dict."""
        if self._net.cond_dim:
            raise NotImplementedError("the latent posterior covers the unconditional 1-layer model only")
        X = np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim)
        return self._net.posterior(X, mask=mask, n_samples=n_samples, n_draws=n_draws, **kwargs)

    def multiple_imputations(self, X, mask, n_samples=5000, n_draws=5, seed=0, **kwargs):
        """Mattei & Frellsen's multiple imputation: n_draws latent vectors per image by SIR from the n_samples importance draws given the
        observed pixels, decoded, the unobserved pixels sampled Bernoulli(sigmoid(l)) on the host (seed), the observed ones put back
        exactly as given.  Returns [n_draws, N, x_dim] float32."""
        X = np.asarray(X, dtype=np.float32).reshape(-1, self._net.x_dim)
        r = self.posterior(X, mask=mask, n_samples=n_samples, n_draws=n_draws, outputs=("z",), **kwargs)
        R, N = int(n_draws), X.shape[0]
        probs = self._net.decode(r["z"].reshape(R * N, -1)).reshape(R, N, -1)
        draws = (np.random.default_rng(seed).random(probs.shape) < probs).astype(np.float32)
        if mask is None:
            return np.ascontiguousarray(np.broadcast_to(X[None], draws.shape))
        return np.where(np.asarray(mask).reshape(X.shape)[None] != 0, X[None], draws).astype(np.float32)
