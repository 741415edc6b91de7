"""Host-side helpers with the reference's names (src/utils.py).  NumPy only; the GPU path never
needs them, they exist so callers written against the reference keep working."""
import os
import numpy as np


def logmeanexp(log_w, axis):
    """src/utils.py:6-8."""
    log_w = np.asarray(log_w)
    m = np.max(log_w, axis=axis)
    return np.log(np.mean(np.exp(log_w - np.expand_dims(m, axis)), axis=axis)) + m


def bernoullisample(x):
    """src/utils.py:26-27 (dynamic binarisation)."""
    return np.random.binomial(1, x, size=x.shape).astype('float32')


def latent_grid(ranges, n):
    """Uniform latent grid in the point order of tasks/plot_task01.py:22-29 (get_grid): a meshgrid of linspaces, so for two dimensions
    the values of one point per grid cell reshape(n2, n1) into the image.  ranges: one (lo, hi) per latent dimension; n: points per
    dimension (an int or one per dimension).  Returns (points [G, D] float32, log_cell_weight [G] float32): the log of the cell volume
    prod_d (hi_d - lo_d) / (n_d - 1), the weight of a Riemann sum of the density over the box."""
    ranges = [tuple(map(float, r)) for r in ranges]
    D = len(ranges)
    ns = [int(n)] * D if np.ndim(n) == 0 else [int(v) for v in n]
    if len(ns) != D or min(ns) < 2:
        raise ValueError("latent_grid: need at least 2 points in each of the %d dimensions" % D)
    axes = [np.linspace(lo, hi, k) for (lo, hi), k in zip(ranges, ns)]
    mesh = np.meshgrid(*axes)
    points = np.stack([m.reshape(-1) for m in mesh], axis=1).astype(np.float32)
    log_cell = float(np.sum([np.log((hi - lo) / (k - 1)) for (lo, hi), k in zip(ranges, ns)]))
    return points, np.full(points.shape[0], log_cell, dtype=np.float32)


class MyMetric():
    """src/utils.py:30-45: list-append mean."""

    def __init__(self):
        self.VALUES = []
        self.N = []

    def update_state(self, losses):
        losses = np.asarray(losses, dtype=np.float32)
        self.VALUES.append(losses.reshape(losses.shape[0], -1) if losses.ndim else losses.reshape(1, 1))
        self.N.append(self.VALUES[-1].shape[0])

    def result(self):
        return np.float32(np.sum(np.concatenate(self.VALUES, axis=0)) / np.float32(np.sum(self.N)))

    def reset_states(self):
        self.VALUES = []
        self.N = []


_MNIST_CANDIDATES = ("IWAE_MNIST_PATH", "~/.keras/datasets/mnist.npz", "./mnist.npz", "./data/mnist.npz")


def count_active(activity, threshold=1e-2):
    """Active units (Burda et al. section 5.2): the number of units whose activity A_u = Cov_x(E_q[u|x]) is strictly above threshold."""
    return int(np.count_nonzero(np.asarray(activity, dtype=np.float64) > threshold))


def _snr_stats(mean, var):
    nz = var > 0
    snr = float(np.mean(np.abs(mean[nz]) / np.sqrt(var[nz]))) if np.any(nz) else float("nan")
    return {"snr": snr, "signal": float(np.sum(mean * mean)), "variance": float(np.sum(var)), "n": int(mean.size)}


def gradient_snr_summary(mean, var, table):
    """Signal-to-noise ratio of a gradient estimator from its per-parameter moments (NativeModel.grad_moments), per tensor of
    `table` (NativeModel.tensor_table(): (name, shape, offset)) and per group: "encoder" = every enc* tensor, "decoder" = every dec*
    tensor.  For each: snr = the mean over the parameters with var > 0 of |mean| / sqrt(var) (Rainforth et al. 2018, averaged; NaN if
    there is none), signal = sum of mean^2, variance = sum of var, n = the parameter count.
    Returns {"encoder": stats, "decoder": stats, "tensors": {name: stats}}."""
    mean = np.asarray(mean, dtype=np.float64).ravel()
    var = np.asarray(var, dtype=np.float64).ravel()
    if mean.shape != var.shape:
        raise ValueError("gradient_snr_summary: mean and var differ in size (%d vs %d)" % (mean.size, var.size))
    tensors, groups = {}, {"encoder": [], "decoder": []}
    for name, shape, off in table:
        sl = slice(int(off), int(off) + int(np.prod(shape)))
        if sl.stop > mean.size:
            raise ValueError("gradient_snr_summary: tensor %s ends at %d, past the %d parameters" % (name, sl.stop, mean.size))
        tensors[name] = _snr_stats(mean[sl], var[sl])
        group = "encoder" if name.startswith("enc") else "decoder" if name.startswith("dec") else None
        if group:
            groups[group].append(sl)
    out = {}
    for group, sls in groups.items():
        idx = np.concatenate([np.arange(sl.start, sl.stop) for sl in sls]) if sls else np.zeros(0, dtype=np.int64)
        out[group] = _snr_stats(mean[idx], var[idx])
    out["tensors"] = tensors
    return out


def find_mnist():
    for c in _MNIST_CANDIDATES:
        p = os.environ.get(c) if c.isupper() else os.path.expanduser(c)
        if p and os.path.exists(p):
            return p
    return None


def load_mnist(path=None):
    """keras.datasets.mnist.load_data() replacement for an offline machine (main.py:59): reads the
    same mnist.npz file Keras caches.  Returns ((Xtrain, ytrain), (Xtest, ytest)) uint8 / None."""
    path = path or find_mnist()
    if path is None:
        return None
    with np.load(path) as f:
        return (f["x_train"], f["y_train"]), (f["x_test"], f["y_test"])


def synthetic_pixel_means(x_dim=784):
    """MNIST-like per-pixel Bernoulli means: smooth centred blob, global mean ~0.13."""
    side = int(round(np.sqrt(x_dim)))
    yy, xx = np.mgrid[0:side, 0:side]
    c = (side - 1) / 2.0
    r2 = ((yy - c) ** 2 + (xx - c) ** 2) / (0.30 * side) ** 2
    return (0.62 * np.exp(-r2)).reshape(-1)[:x_dim]


def synthetic_mnist(n_train=60000, n_test=10000, seed=123, x_dim=784):
    """Grey-level stand-in for MNIST when the real file is absent: per-image intensity-modulated
    blobs in [0,1] (so that dynamic binarisation still has something to sample)."""
    rng = np.random.default_rng(seed)
    p = synthetic_pixel_means(x_dim)[None]

    def make(n):
        scale = rng.uniform(0.5, 1.5, size=(n, 1))
        return np.clip(p * scale, 0.0, 1.0).astype(np.float64)

    return make(n_train), make(n_test)


def bias_from_mean(train_mean):
    """src/utils.py:19-21."""
    return (-np.log(1. / np.clip(np.asarray(train_mean, dtype=np.float64), 0.001, 0.999) - 1.)).astype(np.float32)


def get_bias(Xtrain=None):
    """src/utils.py:11-23: logit of the clipped per-pixel training mean.  The reference downloads
    MNIST here; offline we take the training matrix from the caller or a local mnist.npz."""
    if Xtrain is None:
        data = load_mnist()
        if data is None:
            raise FileNotFoundError("get_bias(): no local mnist.npz (set IWAE_MNIST_PATH) and no Xtrain given")
        Xtrain = data[0][0]
    Xtrain = np.asarray(Xtrain)
    Xtrain = Xtrain.reshape(Xtrain.shape[0], -1)
    if Xtrain.dtype == np.uint8:
        Xtrain = Xtrain / 255
    return bias_from_mean(np.mean(Xtrain, axis=0))


def mean_se(log_w):
    """Standard error of the mean over axis 0 (the E S evaluation draws of iwae_local_posterior's log_w [E S, N]) per image, float64."""
    lw = np.asarray(log_w, dtype=np.float64)
    return lw.std(axis=0, ddof=1) / np.sqrt(lw.shape[0]) if lw.shape[0] > 1 else np.full(lw.shape[1:], np.nan)


def log_mean_exp_se(log_w):
    """Delta-method standard error of log mean_c exp(log_w) over axis 0 per image: std(w) / (mean(w) sqrt(C))."""
    lw = np.asarray(log_w, dtype=np.float64)
    if lw.shape[0] < 2:
        return np.full(lw.shape[1:], np.nan)
    w = np.exp(lw - lw.max(axis=0)[None])
    return w.std(axis=0, ddof=1) / (w.mean(axis=0) * np.sqrt(lw.shape[0]))


def inference_gap_split(log_px, elbo_amortized, elbo_local):
    """Cremer, Li & Duvenaud (2018): log p(x) - ELBO[q_enc] = (log p(x) - ELBO[q*]) + (ELBO[q*] - ELBO[q_enc]), per image in float64."""
    lp, ea, el = (np.asarray(v, dtype=np.float64) for v in (log_px, elbo_amortized, elbo_local))
    return {"log_px": lp, "elbo_amortized": ea, "elbo_local": el, "approximation_gap": lp - el, "amortization_gap": el - ea}


def mcar_mask(shape, rate, seed=0):
    """A missing-completely-at-random mask for iwae_impute: uint8 array of `shape`, 1 = observed, each entry unobserved with probability
    `rate` independently (seeded host generator)."""
    if not 0.0 <= rate <= 1.0:
        raise ValueError("mcar_mask: rate must lie in [0, 1], got %r" % (rate,))
    return (np.random.default_rng(seed).random(shape) >= rate).astype(np.uint8)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays of uint32 counters under one key; four uint32 arrays."""
    c0, c1, c2, c3 = [np.array(c, dtype=np.uint32) for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    lo32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0.astype(np.uint64)
        p1 = np.uint64(0xCD9E8D57) * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & lo32).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & lo32).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def mcar_threshold(rate):
    """The integer threshold of the device mask generator: floor(rate 2^24 + 0.5), in double."""
    rate = float(rate)
    if not 0.0 <= rate <= 1.0:      # (NaN fails both comparisons)
        raise ValueError("mcar mask: rate must lie in [0, 1], got %r" % (rate,))
    return int(np.floor(rate * 16777216.0 + 0.5))


def device_mcar_mask(n, x_dim, rate, seed=0):
    """The masks iwae_dataset_mcar_mask draws for an n-image set, bit for bit: uint8 [n, x_dim], 1 = observed.  Pixel f of image i is
    hidden iff (philox4x32_10(counter = (i, 'MASK', f >> 2, 0), key = (seed lo, seed hi))[f & 3] >> 8) < floor(rate 2^24 + 0.5)."""
    thr = mcar_threshold(rate)
    n, x_dim, seed = int(n), int(x_dim), int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (x_dim + 3) // 4
    c0 = np.broadcast_to(np.arange(n, dtype=np.uint32)[:, None], (n, nq))
    c2 = np.broadcast_to(np.arange(nq, dtype=np.uint32)[None, :], (n, nq))
    r = _philox4x32_10(c0, np.uint32(0x4D41534B), c2, np.uint32(0), seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack([w >> np.uint32(8) for w in r], axis=-1).reshape(n, 4 * nq)[:, :x_dim]
    return (u.astype(np.int64) >= thr).astype(np.uint8)
