"""numpy restatement of iwae_impute's formulas (include/iwae_amd.h), in the dtype given, and the inputs of its parity cases: shared by
tests/test_impute_host.py and tests/test_gpu_impute.py.  Not a test module.

Built on tests/_ais_ref.py's decoder_of / logits_of.  Unobserved pixels are removed with np.where, never multiplied by the mask, so a
NaN in x at such a pixel reaches nothing."""
import numpy as np

from oracle import iwae_np as O
import make_golden as MG
import _ais_ref as R
import _parity_common as PC

HALF_LOG_2PI = R.HALF_LOG_2PI

SHAPES = [(64, 8, 48), (200, 100, 784), (37, 5, 53)]
NMAX = 5
# (N, k): one row | dead rows in a wave | images straddle waves | two workgroups | exactly one image per workgroup | an image in two chunks |
# five chunks | several images of two chunks each
CASES = [(1, 1), (1, 17), (3, 7), (5, 13), (2, 64), (2, 65), (1, 257), (5, 70)]
CASE_IDS = ["row", "dead", "straddle", "two_wg", "one_image", "two_chunks", "five_chunks", "images_of_chunks"]


def shape_inputs(nh, nl, xd):
    """The images, the SPREAD parameters (tests/_parity_common.py: the weights over an image's draws are not one-hot) and the 50 % mask of
    one shape: x [NMAX, xd] float32, P, mask [NMAX, xd] bool."""
    x, P, _ = MG.inputs(1, nh, nl, xd, NMAX, 1, 7 + nh)
    mask = np.random.default_rng(1000 + nh).random((NMAX, xd)) < 0.5
    return x, PC.spread_params(P, 1), mask


def draws(N, k, nl):
    return np.random.default_rng(100 + 10 * N + k).standard_normal((k, N, nl)).astype(np.float32)


def encoder_heads(P, x, mask):
    """mu, sigma [N, D] of the encoder (src/iwae1.py:39-42) at the masked input m ? x : 0, float64."""
    xin = np.where(mask, np.asarray(x, dtype=np.float64), 0.0)
    return O._Block(P[0:4], O._id).fwd(xin)


def restate(P, x, mask, mu, sigma, eps, dtype=np.float64):
    """x [N, X]; mask [N, X] (non-zero = observed) or None; mu, sigma [N, D]; eps [k, N, D].  Every product and sum in `dtype` except log_px
    (float64 over the `dtype` log_w, as the device).  Returns log_w [k, N], log_px [N] (float64), ess [N], al [k, N], p [k, N, X], xhat [N, X]."""
    dt = np.dtype(dtype).type
    dec = R.decoder_of(P, dtype)
    e = np.asarray(eps, dtype=dtype)
    k, N, D = e.shape
    mu, sigma = np.asarray(mu, dtype=dtype), np.asarray(sigma, dtype=dtype)
    obs = np.ones(np.shape(x), dtype=bool) if mask is None else np.asarray(mask) != 0
    xs = np.where(obs, np.asarray(x, dtype=dtype), dt(0))              # selected, not multiplied
    z = mu[None] + sigma[None] * e
    l = R.logits_of(dec, z.reshape(k * N, D))[2].reshape(k, N, -1)
    ex = np.exp(-np.abs(l))
    terms = xs[None] * l - (np.maximum(l, dt(0)) + np.log1p(ex))
    lpx = np.sum(np.where(obs[None], terms, dt(0)), axis=-1)
    lpz = np.sum(dt(-0.5) * z * z - dt(HALF_LOG_2PI), axis=-1)
    lq = np.sum(dt(-0.5) * e * e - np.log(sigma)[None] - dt(HALF_LOG_2PI), axis=-1)
    log_w = lpx + lpz - lq
    mx = log_w.max(axis=0)
    w = np.exp(log_w - mx[None])
    al = w / w.sum(axis=0, keepdims=True)
    lw64 = log_w.astype(np.float64)
    m64 = lw64.max(axis=0)
    log_px = m64 + np.log(np.sum(np.exp(lw64 - m64[None]), axis=0)) - np.log(k)
    p = np.where(l >= 0, dt(1) / (dt(1) + ex), ex / (dt(1) + ex))
    xhat = np.sum(al[:, :, None] * p, axis=0)
    return {"log_w": log_w, "log_px": log_px, "ess": dt(1) / np.sum(al * al, axis=0), "al": al, "p": p, "xhat": xhat,
            "lpz_minus_lq": lpz - lq}


def quadrature_log_px_obs(P, x, mask, n=401, extent=8.0):
    """log p(x_obs) of a model with TWO latent dimensions by the rectangle rule on an n x n grid over [-extent, extent]^2 (float64): the
    observed pixels' Bernoulli terms times the N(0, I) prior (tests/_ais_ref.py's quadrature_log_px with the unobserved pixels left out)."""
    dec = R.decoder_of(P, np.float64)
    g = np.linspace(-extent, extent, n)
    lw = 2.0 * np.log(g[1] - g[0])
    obs = np.asarray(mask) != 0
    xs = np.where(obs, np.asarray(x, dtype=np.float64), 0.0)
    run = np.full(xs.shape[0], -np.inf)
    for i in range(0, n, 50):
        zz = np.stack(np.meshgrid(g[i:i + 50], g, indexing="ij"), axis=-1).reshape(-1, 2)
        l = R.logits_of(dec, zz)[2]                                       # [G, X]
        sp = np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l)))
        lj = xs @ l.T - obs.astype(np.float64) @ sp.T                      # (0/1 weights of exact terms: which pixels enter)
        lj = lj + (-0.5 * np.sum(zz * zz, axis=1) - 2 * HALF_LOG_2PI)[None] + lw
        m = np.maximum(run, lj.max(axis=1))
        run = m + np.log(np.exp(run - m) + np.sum(np.exp(lj - m[:, None]), axis=1))
    return run
