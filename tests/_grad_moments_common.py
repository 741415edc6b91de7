"""Helpers of the iwae_grad_moments GPU tests (tests/test_gpu_grad_moments.py, tests/test_gpu_ragged_widths.py): the seeded set-up, the
float64 Welford fold over per-draw gradients and the state / closeness checks.  Not a test module."""
import numpy as np

from oracle import iwae_np as O
import make_golden as MG

S0 = 11


def _model(layers, nh, nl, xd, prec, B, k, cond=0, seed=100, options=None):
    from iwae_amd.native import NativeModel
    if cond:
        x, P, _, y = MG.inputs(layers, nh, nl, xd, B, k, seed, cond=cond)
    else:
        (x, P, _), y = MG.inputs(layers, nh, nl, xd, B, k, seed), None
    m = NativeModel(layers, nh, nl, x_dim=xd, seed=123, cond_dim=cond, precision=prec, options=options)
    m.set_params(O.flatten_params(P))
    if cond:
        m.set_condition(y)
    rng = np.random.default_rng(seed + 1)       # a non-trivial optimizer state, to see that the call leaves it alone
    m.set_adam_state(rng.standard_normal(m.n_params).astype(np.float32) * 1e-3,
                     rng.random(m.n_params).astype(np.float32) * 1e-6, 7)
    return m, x, P, y


class _Welford:
    """The float64 reference fold: mean += (g - mean) / j, M2 += (g - mean_old)(g - mean_new)."""

    def __init__(self):
        self.j, self.mean, self.m2 = 0, None, None

    def add(self, g):
        g = np.asarray(g, dtype=np.float64)
        self.j += 1
        if self.j == 1:
            self.mean, self.m2 = g.copy(), np.zeros_like(g)
            return
        d = g - self.mean
        self.mean = self.mean + d / self.j
        self.m2 = self.m2 + d * (g - self.mean)

    def var(self):
        return self.m2 / (self.j - 1)


def _host_fold(m, x, k, beta, obj, s0, M):
    w = _Welford()
    for j in range(M):
        m.set_step(s0 + j)
        m.forward_backward(x, k, beta, obj)
        g = m.get_grads()
        w.add(g)
    return w.mean, w.var(), g


def _state(m):
    mo, ve, t = m.get_adam_state()
    return m.get_params(), mo, ve, t


def _assert_state_equal(a, b):
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert a[3] == b[3]


def _close(got, want, rtol=1e-12):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * float(np.max(np.abs(want))) + 1e-300)
