"""Shared by test_adam_host.py and test_gpu_adam.py: the float64 reference of the device's Adam update (adam_math in update_kernels.hip, the one
function inlined into adam_kernel, reduce_grads_kernel and wgrad_rows_kernel), per-element error bounds for it, constructed inputs and the
hyper-parameter cases.

The update is elementwise in float32, so its error is bounded from the number of roundings, not from a measurement.  With u = 2^-24,
per element (adam_excess returns max |error| / bound for each of m, v, w; a check passes iff every figure is <= 1):

  m:  |m_dev - m64| <= 4u (|b1 m_old| + |(1 - b1) g gs|)
        the roundings of g gs, 1 - b1, the product and the fused multiply-add are <= 2u of those two terms; written on the TERMS the bound
        survives cancellation between m_old and g (a bound relative to m64 does not).
  v:  |v_dev - v64| <= 8u v64
        all terms are positive; g gs enters twice, then 1 - b2, two products and the fused multiply-add.
  w:  |w_dev - (w_old - q64)| <= u (8 |q64| + |w_old| + |w_new|),   q64 = alpha m_dev / (sqrt(v_dev) + eps) in float64
        the step is evaluated at the DEVICE's own new m and v (the suite's "at the device's own heads" idiom): product, square root, sum and
        quotient are 4-5u relative in q, the final subtraction half an ulp of w.
  exact rule: an element with g == 0, m_old == 0 and v_old == 0 keeps w bitwise and leaves m = v = 0.

A float32 NumPy restatement without fused multiply-adds stays below 0.5 / 0.5 / 0.85 of these bounds on every hyper-parameter case
(test_adam_host.py), so they are admissible from the reference alone; the constants are never fitted to a device run.

The hyper-parameters are the values the device RECEIVES: b1, b2, eps, gs and lr rounded to float32 (the C ABI takes floats), then widened.
alpha = float32(lr sqrt(1 - b2^t) / (1 - b1^t)) evaluated in double, as adam_alpha (model.hip) does; t is the step count AFTER the increment.
"""
import collections

import numpy as np

U = 2.0 ** -24
M_BOUND, V_BOUND, Q_BOUND = 4.0, 8.0, 8.0

HyperCase = collections.namedtuple("HyperCase", "id b1 b2 eps t0 gscale lr fresh")

# (id, b1, b2, eps, t before the step, grad_scale, lr, fresh state)
HYPER_CASES = [
    HyperCase("A", 0.9, 0.999, 1e-4, 0, 1.0, 1e-3, True),                # fresh state, the reference's hyper-parameters
    HyperCase("B", 0.9, 0.999, 1e-4, 99999, 1.0 / 8.0, 1e-3, False),     # resumed run (bias correction ~ 1), the 8-rank gradient scale
    HyperCase("C", 0.9, 0.999, 1e-7, 1999, 1.0, 1e-3, False),            # optimizers.Adam's Keras default epsilon
    HyperCase("D", 0.5, 0.9, 1e-7, 6, 1.0 / 3.0, 1e-2, False),           # inexact gradient scale, non-default betas
    HyperCase("E", 0.0, 0.0, 1e-4, 2, 1.0, 1e-3, False),                 # the edges iwae_set_adam admits: m = g gs, v = (g gs)^2
    HyperCase("F", 0.9, 0.999, 1e-4, 9999999, 1.0, 1e-4, False),         # beta^t underflows: alpha == float32(lr) exactly
    HyperCase("G", 0.9, 0.999, 1e-4, 5, 1.0, 0.0, False),                # lr = 0: w bitwise unchanged, m, v, t advance
]
CASE = {c.id: c for c in HYPER_CASES}


def f32(x):
    """x rounded to float32 and widened again: the value the device receives for a float argument."""
    return float(np.float32(x))


def adam_alpha(t, lr, b1, b2):
    """adam_alpha of model.hip: the bias-corrected step size of step t (counted after the increment), evaluated in double from the float32
    hyper-parameters and rounded to float32 once."""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return float(np.float32(lr * np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))))


def adam_ref64(w, g, m, v, t, lr, b1, b2, eps, gscale):
    """float64 Keras Adam (epsilon outside the square root) on float32 inputs.  Returns (w, m, v) after the step, float64."""
    w, g, m, v = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v))
    b1, b2, eps, gs = f32(b1), f32(b2), f32(eps), f32(gscale)
    alpha = adam_alpha(t, lr, b1, b2)
    g = g * gs
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return w - alpha * m / (np.sqrt(v) + eps), m, v


def _worst(err, bound):
    """max err / bound; a zero bound admits a zero error only."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def adam_excess(w, g, m, v, t, lr, b1, b2, eps, gscale, w_dev, m_dev, v_dev):
    """The three figures (m, v, w) of the module docstring for one step from (w, g, m, v) to the device's (w_dev, m_dev, v_dev).
    A non-finite device value gives inf."""
    w, g, m, v, w_dev, m_dev, v_dev = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v, w_dev, m_dev, v_dev))
    if not (np.isfinite(w_dev).all() and np.isfinite(m_dev).all() and np.isfinite(v_dev).all()):
        return float("inf"), float("inf"), float("inf")
    _, m64, v64 = adam_ref64(w, g, m, v, t, lr, b1, b2, eps, gscale)
    b1f, gs = f32(b1), f32(gscale)
    fm = _worst(np.abs(m_dev - m64), M_BOUND * U * (np.abs(b1f * m) + np.abs((1.0 - b1f) * g * gs)))
    fv = _worst(np.abs(v_dev - v64), V_BOUND * U * v64)
    q64 = adam_alpha(t, lr, b1, b2) * m_dev / (np.sqrt(v_dev) + f32(eps))
    fw = _worst(np.abs(w_dev - (w - q64)), U * (Q_BOUND * np.abs(q64) + np.abs(w) + np.abs(w_dev)))
    return fm, fv, fw


def exact_rule_violations(w, g, m, v, w_dev, m_dev, v_dev):
    """(number of elements with g == 0, m_old == 0 and v_old == 0, how many of them moved: w not bitwise kept, or m, v not 0)."""
    w, w_dev = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(w_dev, dtype=np.float32)
    still = (np.asarray(g) == 0) & (np.asarray(m) == 0) & (np.asarray(v) == 0)
    bad = still & ((w.view(np.uint32) != w_dev.view(np.uint32)) | (np.asarray(m_dev) != 0) | (np.asarray(v_dev) != 0))
    return int(still.sum()), int(bad.sum())


def adam_inputs(n, seed, fresh=False):
    """Constructed (w, g, m, v) of n float32 elements that cover the update's regimes:
      g = N(0,1) 10^U(-12, 2): from far below every epsilon to far above; exactly 0 on the first 1 % of the elements, elsewhere
          |g| >= 1e-13 so that every product of the update stays a normal float32 (denormal handling is not under test);
      m = N(0,1) 10^U(-8, 0), v = 10^U(-16, 2): sqrt(v) from 1e-8 (epsilon dominates) to 10 (epsilon vanishes), independent of m
          (cancellation between b1 m and (1 - b1) g happens);  fresh: m = v = 0;
      w = N(0,1) 10^U(-3, 0).
    Every second element of the zero-g block also has m = v = 0: the exact rule's elements."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-12.0, 2.0, n)
    g = np.where(np.abs(g) < 1e-13, np.copysign(1e-13, g), g)
    m = rng.standard_normal(n) * 10.0 ** rng.uniform(-8.0, 0.0, n)
    v = 10.0 ** rng.uniform(-16.0, 2.0, n)
    w = rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 0.0, n)
    nz = max(2, (n + 99) // 100)
    g[:nz] = 0.0
    if fresh:
        m[:] = 0.0
        v[:] = 0.0
    m[:nz:2] = 0.0
    v[:nz:2] = 0.0
    return tuple(a.astype(np.float32) for a in (w, g, m, v))


def plausible_state(m, v):
    """(m, v) with v raised to m^2 where it is smaller (and to 1e-16 where it is 0): |m| / sqrt(v) <= 1, as in every state Adam itself
    produces, so a step moves no weight by more than ~alpha and a forward pass after it stays finite.  Used where the stepped parameters
    are run through the model; sqrt(v) still spans 1e-8 .. 10."""
    m = np.asarray(m, dtype=np.float32)
    v = np.maximum(np.maximum(np.asarray(v, dtype=np.float32), m * m), np.float32(1e-16))
    return m, v


def adam_math_f32(w, g, m, v, alpha, b1, b2, eps, gscale, mutation=None, trace=None):
    """adam_math restated in float32 NumPy, one rounding per operation and NO fused multiply-add (so it is not bit-equal to the device:
    it shows that an honest float32 evaluation sits inside the bounds).  mutation: one of MUTATIONS, a deliberate error the bounds must
    see.  trace: a list that receives every intermediate array."""
    F = np.float32
    w, g, m, v = (np.asarray(a, dtype=F) for a in (w, g, m, v))
    alpha, b1, b2, eps, gs = F(alpha), F(b1), F(b2), F(eps), F(gscale)
    keep = (lambda a: (trace.append(a), a)[1]) if trace is not None else (lambda a: a)
    one = F(1.0)
    gg = keep(g * gs)
    bm = b2 if mutation == "beta2_for_m" else b1
    m = keep(keep(bm * m) + keep(keep(one - bm) * gg))
    g2 = g if mutation == "scale_not_squared" else gg          # grad_scale applied to g but not to g * g
    v = keep(keep(b2 * v) + keep(keep(keep(one - b2) * g2) * g2))
    den = keep(np.sqrt(keep(v + eps))) if mutation == "eps_inside_root" else keep(keep(np.sqrt(v)) + eps)
    q = keep(keep(alpha * m) / den)
    return keep(w - q), m, v


MUTATIONS = ("eps_inside_root", "scale_not_squared", "no_bias_correction", "beta2_for_m")
