"""Host checks of the Adam reference and bounds of _adam_ref.py (no GPU): the reference is the project's oracle, an honest float32
evaluation of adam_math sits well inside the bounds on every hyper-parameter case, never leaves the normal float32 range on the constructed
inputs, and the bounds are tight enough to see four classic mistakes."""
import numpy as np
import pytest

from oracle import iwae_np as O
import _adam_ref as R

N = 400_000


def _case_inputs(c):
    return R.adam_inputs(N, 10 + ord(c.id), c.fresh)


@pytest.mark.parametrize("fresh,t", [(True, 1), (False, 2), (False, 2000), (False, 100000)])
def test_reference_is_the_oracles_adam_update(fresh, t):
    """adam_ref64 at the default hyper-parameters against oracle.iwae_np.adam_update given the same float32-rounded hyper-parameters: the
    parameter change agrees to 1e-7 relative per element (what is left is the one float32 rounding of alpha, <= 2^-24 = 6e-8).  The change is
    taken from w = 0 so that no cancellation against w enters the comparison.
    (Given the DECIMAL hyper-parameters the oracle differs by 6.4e-6 relative: float32(0.999) moves 1 - b2 by 1.3e-5 of itself, and half
    of that reaches sqrt(v) -- the rounding the device's arguments have, which is why the reference rounds them first.)"""
    _, g, m, v = R.adam_inputs(N, 3, fresh)
    w = np.zeros(N, dtype=np.float32)
    lr, b1, b2, eps = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-4)
    w64, m64, v64 = R.adam_ref64(w, g, m, v, t, 1e-3, 0.9, 0.999, 1e-4, 1.0)
    wo, mo, vo = O.adam_update(w.astype(np.float64), g.astype(np.float64), m.astype(np.float64), v.astype(np.float64), t, lr, b1, b2, eps)
    np.testing.assert_array_equal(m64, mo)
    np.testing.assert_array_equal(v64, vo)
    d = np.abs(w64 - wo)
    worst = float(np.max(d[wo != 0] / np.abs(wo[wo != 0])))
    print("adam_ref64 vs oracle, t = %d: worst relative deviation of the change %.3g" % (t, worst))
    assert worst <= 1e-7
    assert np.all(d[wo == 0] == 0)


def test_alpha_edges():
    """beta^t underflows at t = 1e7: alpha is float32(lr) exactly; lr = 0 gives alpha = 0; betas of 0 need no correction."""
    assert R.adam_alpha(10_000_000, 1e-4, 0.9, 0.999) == float(np.float32(1e-4))
    assert R.adam_alpha(6, 0.0, 0.9, 0.999) == 0.0
    assert R.adam_alpha(3, 1e-3, 0.0, 0.0) == float(np.float32(1e-3))


@pytest.mark.parametrize("c", R.HYPER_CASES, ids=[c.id for c in R.HYPER_CASES])
def test_float32_restatement_is_inside_the_bounds(c):
    """adam_math restated in float32 NumPy (no fused multiply-add) stays below 0.5 / 0.5 / 0.85 of the m / v / w bounds, obeys the exact
    rule, and every intermediate is 0 or a normal float32: the bounds follow from the arithmetic, and the inputs test no denormal."""
    w, g, m, v = _case_inputs(c)
    t = c.t0 + 1
    trace = []
    wd, md, vd = R.adam_math_f32(w, g, m, v, R.adam_alpha(t, c.lr, c.b1, c.b2), c.b1, c.b2, c.eps, c.gscale, trace=trace)
    fm, fv, fw = R.adam_excess(w, g, m, v, t, c.lr, c.b1, c.b2, c.eps, c.gscale, wd, md, vd)
    print("case %s float32 restatement: m %.3f / 1, v %.3f / 1, w %.3f / 1" % (c.id, fm, fv, fw))
    assert fm <= 0.5 and fv <= 0.5 and fw <= 0.85, (fm, fv, fw)
    n_still, n_bad = R.exact_rule_violations(w, g, m, v, wd, md, vd)
    assert n_still >= N // 200 and n_bad == 0
    tiny = np.finfo(np.float32).tiny
    for a in trace:
        a = np.abs(np.asarray(a))
        assert np.all(np.isfinite(a)) and np.all((a == 0) | (a >= tiny))
    if c.id == "G":
        np.testing.assert_array_equal(wd.view(np.uint32), w.view(np.uint32))
        assert np.any(md != m) and np.any(vd != v)
    if c.id == "E":      # b1 = b2 = 0: the state forgets itself
        np.testing.assert_array_equal(md, g)
        np.testing.assert_array_equal(vd, g * g)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("cid", ["B", "D"])
def test_bounds_see_a_mutated_update(cid, mutation):
    """Each deliberate error in the float32 restatement pushes a figure above 1 (the omitted bias correction is run at t = 7, where it
    matters; at case B's own t = 1e5 the correction IS 1)."""
    c = R.CASE[cid]
    w, g, m, v = _case_inputs(c)
    t = 7 if mutation == "no_bias_correction" else c.t0 + 1
    alpha = R.f32(c.lr) if mutation == "no_bias_correction" else R.adam_alpha(t, c.lr, c.b1, c.b2)
    wd, md, vd = R.adam_math_f32(w, g, m, v, alpha, c.b1, c.b2, c.eps, c.gscale, mutation=mutation)
    fm, fv, fw = R.adam_excess(w, g, m, v, t, c.lr, c.b1, c.b2, c.eps, c.gscale, wd, md, vd)
    print("case %s, %s: m %.3g, v %.3g, w %.3g" % (cid, mutation, fm, fv, fw))
    assert max(fm, fv, fw) > 1.0
    # ... and it is that mutation's own figure that moves
    own = {"eps_inside_root": fw, "scale_not_squared": fv, "no_bias_correction": fw, "beta2_for_m": fm}[mutation]
    assert own > 1.0


def test_inputs_cover_the_regimes():
    """adam_inputs reaches both ends: epsilon dominates sqrt(v) and vanishes beside it, for both epsilons in use; the exact-rule block exists."""
    w, g, m, v = R.adam_inputs(N, 5)
    s = np.sqrt(v[v > 0].astype(np.float64))
    assert (s < 0.2 * 1e-7).any() and (s < 1e-2 * 1e-4).any() and (s > 1e4 * 1e-4).any()
    nz = (N + 99) // 100
    assert np.all(g[:nz] == 0) and np.all(g[nz:] != 0) and np.min(np.abs(g[nz:])) >= np.float32(1e-13)
    assert np.all(m[:nz:2] == 0) and np.all(v[:nz:2] == 0) and np.all(v[1:nz:2] > 0)
    _, _, mf, vf = R.adam_inputs(1000, 5, fresh=True)
    assert not mf.any() and not vf.any()
    mp, vp = R.plausible_state(m, v)
    assert np.all(vp > 0) and np.all(np.abs(mp) <= np.sqrt(vp.astype(np.float64)) * (1 + 1e-6))
