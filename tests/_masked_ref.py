"""The masked train step (iwae_forward_masked / iwae_forward_backward_masked / iwae_train_step_masked, include/iwae_amd.h; Mattei &
Frellsen 2019) restated in float64 torch autograd -- shared by test_masked_host.py and test_gpu_masked_step.py; not a test module.

Built from oracle/iwae_torch.py's own pieces (_block, _mlp3, _normal_lp, _bern_lp, _logmeanexp) with torch.where on the mask in the three
places the masked step differs from the unmasked one: the encoder reads xin = m ? x : 0, log p(x|z) sums the observed pixels' Bernoulli
terms, and -- through autograd -- the backward pass starts from s = m ? x - sigmoid(l) : 0.  The objectives follow forward_1layer line by
line, DReG follows loss_grads.  torch.where SELECTS: what x holds where m = 0 never enters a product.
"""
import functools

import numpy as np
import torch

from oracle import iwae_np as O
from oracle import iwae_torch as T
import make_golden as MG
from _parity_common import spread_params

OBJECTIVES = ("iwae_elbo", "vae_elbo", "dreg")
SHAPES = [(200, 100, 784), (16, 4, 48), (208, 128, 800), (37, 5, 53)]      # (n_hidden, n_latent, x_dim); the third: the widest the fast route takes
FAST_SHAPES = SHAPES[:3]                                                    # 37 / 5 / 53: x_dim no multiple of 4, the general route only
# (B, k): one row; three images in a wave; (20, 1) more than three images in a wave; (5, 13) = 65 rows: the second workgroup holds one row;
# two images of a whole workgroup each; one image over three workgroups
CASES = [(1, 1), (3, 7), (20, 1), (5, 13), (2, 64), (1, 130)]
# default options; 10 000 rows: past the unmasked plan's fused-epilogue threshold; 25 600 rows: masked_out_min_rows' default, the fast route unforced
BIG_CASES = [(82, 50), (200, 50), (512, 50)]
ROUTES = {"general": {"no_masked_out_fused": 1}, "fast": {"masked_out_min_rows": 1}}


def masked_forward(params, x, mask, eps, beta=1.0, dreg=False):
    """forward_1layer of oracle/iwae_torch.py with the mask; params / x / eps torch float64, mask a torch bool array [B, X]."""
    zero = torch.zeros((), dtype=x.dtype)
    xin = torch.where(mask, x, zero)
    mu, sigma = T._block(params[0:4], xin)
    z = mu.unsqueeze(0) + sigma.unsqueeze(0) * eps
    logits = T._mlp3(params[4:7], z)
    lpz = T._normal_lp(z, torch.zeros((), dtype=z.dtype), torch.ones((), dtype=z.dtype)).sum(-1)
    lqzx = T._normal_lp(z, mu.unsqueeze(0), sigma.unsqueeze(0)).sum(-1)
    lpxz = torch.where(mask.unsqueeze(0), T._bern_lp(xin.unsqueeze(0), logits), zero).sum(-1)
    log_w = lpxz + beta * (lpz - lqzx)
    ls = torch.log(sigma)
    kl = (0.5 * mu * mu + 0.5 * torch.expm1(2.0 * ls) - ls).sum(-1)
    res = {}
    res["vae_elbo"] = log_w.mean(0).mean(-1)
    res["vae_elbo_kl"] = lpxz.mean() - beta * kl.mean()
    res["iwae_elbo"] = T._logmeanexp(log_w, 0).mean(-1)
    m = log_w.max(dim=0, keepdim=True).values
    w = torch.exp(log_w - m)
    wn = (w / w.sum(0, keepdim=True)).detach()
    res["iwae_eq14"] = (wn * log_w).sum(0).mean()
    al = torch.softmax(log_w, dim=0)
    res["snis_z"] = (al.unsqueeze(-1) * z).sum(0)
    res.update(z=z, al=al, logits=logits, lpxz=lpxz, lpz=lpz, lqzx=lqzx, log_w=log_w)
    if dreg:
        mu_s, sig_s = mu.detach(), sigma.detach()
        lq_st = T._normal_lp(z, mu_s.unsqueeze(0), (sig_s + T.SIGMA_EPS).unsqueeze(0)).sum(-1)
        sq = al.detach() ** 2
        res["inference_loss"] = -((sq * (lpz + lpxz - lq_st)).sum(0)).mean(-1)
    return res


def masked_loss_grads(params_np, x, mask, eps, beta=1.0, objective="iwae_elbo"):
    """loss_grads of oracle/iwae_torch.py for the masked step: (res, [(dW, db) ...]) as float64 numpy."""
    P = T.to_torch_params(params_np, torch.float64)
    xt = torch.tensor(np.asarray(x), dtype=torch.float64)
    mt = torch.tensor(np.asarray(mask) != 0)
    e = torch.tensor(np.asarray(eps), dtype=torch.float64)
    flatP = [t for Wb in P for t in Wb]
    if objective == "dreg":
        res = masked_forward(P, xt, mt, e, beta, dreg=True)
        enc = [t for Wb in P[0:4] for t in Wb]
        dec = [t for Wb in P[4:7] for t in Wb]
        ge = torch.autograd.grad(res["inference_loss"], enc, retain_graph=True)
        gd = torch.autograd.grad(-res["iwae_elbo"], dec)
        g = list(ge) + list(gd)
    else:
        res = masked_forward(P, xt, mt, e, beta)
        g = torch.autograd.grad(-res[objective], flatP, allow_unused=True)
        g = [gi if gi is not None else torch.zeros_like(p) for gi, p in zip(g, flatP)]
    grads = [(g[2 * i].numpy(), g[2 * i + 1].numpy()) for i in range(len(P))]
    return {k_: v.detach().numpy() for k_, v in res.items()}, grads


def case_mask(B, X, seed):
    """A 50 % MCAR mask [B, X] (uint8, 1 = observed) in which, where the batch has the images for it, the first image has nothing observed
    (B >= 2), the second only its last pixel (B >= 3: the last pixel tile then holds a single live column) and the last is fully observed
    (B >= 4); at least one image always keeps its MCAR row."""
    from iwae_amd.utils import mcar_mask
    m = mcar_mask((B, X), 0.5, seed=seed)
    if B >= 2:
        m[0] = 0
    if B >= 3:
        m[1] = 0
        m[1, X - 1] = 1
    if B >= 4:
        m[B - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(nh, nl, xd, B, k):
    """(x, P, eps, mask) of a case: make_golden.inputs, spread_params (the weights over an image's samples are not one-hot) and case_mask."""
    x, P, eps = MG.inputs(1, nh, nl, xd, B, k, 900 + B + k)
    return x, spread_params(P, 1), eps, case_mask(B, xd, 17 + B + k)


@functools.lru_cache(maxsize=None)
def reference(nh, nl, xd, B, k, objective, beta=1.0):
    """masked_loss_grads of a case, computed once and shared; read only."""
    x, P, eps, mask = case(nh, nl, xd, B, k)
    return masked_loss_grads(P, x, mask, eps, beta, objective)


def masked_out_launches(m, call):
    """(call(), launches of masked_out_f32_kernel while it ran): iwae_enable_timing(1) zeroes the counters, iwae_kernel_time(h, "masked_out")
    reads the launch count -- the one witness of which route of the output layer a masked call took (plan_step_f32 falls back to the general
    route silently where masked_out_f32_ok refuses).  Timing is switched off again; the events change no result."""
    m.enable_timing(1)
    try:
        out = call()
        launches = m.kernel_time("masked_out")[1]
    finally:
        m.enable_timing(0)
    return out, launches


def expected_on_fast_route(route, launches, rows=0):
    """The witness against the route a test names: "fast..." > 0 launches, "general..." 0, "default" the fast route from 25 600 rows."""
    fast = route.startswith("fast") or (route == "default" and rows >= 25600)
    assert (launches > 0) == fast, "route %r at %d rows: %d launches of masked_out_f32_kernel" % (route, rows, launches)


def sliced_oracle_grads(P, x, mask, eps, beta, objective, rnd=None):
    """The masked step through the committed NumPy oracle alone: image by image (B = 1), on the model whose encoder has lost the unobserved
    rows of its first kernel and whose decoder has lost the unobserved columns of W3 / b3; the gradients scattered back and averaged over
    the images.  rnd: the oracle's rounding hook (None: exact float64; _offinit_cases.f32_round: every operand rounded to float32).  Returns
    ({objective value, lpxz / lpz / lqzx / al [k, B]}, [(dW, db) ...])."""
    B = x.shape[0]
    acc = [(np.zeros_like(W), np.zeros_like(b)) for W, b in P]
    val, rows = 0.0, {key: [] for key in ("lpxz", "lpz", "lqzx", "al")}
    for b_ in range(B):
        obs = np.flatnonzero(mask[b_])
        Ps = [(np.array(W), np.array(b)) for W, b in P]
        Ps[0] = (P[0][0][obs, :], P[0][1])
        Ps[6] = (P[6][0][:, obs], P[6][1][obs])
        res, g = O.loss_grads_1layer(Ps, x[b_:b_ + 1, obs], eps[:, b_:b_ + 1, :], beta, objective, rnd=rnd)
        val += float(res["iwae_elbo" if objective == "dreg" else objective]) / B
        for key in rows:
            rows[key].append(res[key][:, 0])
        for i, (dW, db) in enumerate(g):
            if i == 0:
                acc[0][0][obs, :] += dW / B
                acc[0][1][:] += db / B
            elif i == 6:
                acc[6][0][:, obs] += dW / B
                acc[6][1][obs] += db / B
            else:
                acc[i][0][:] += dW / B
                acc[i][1][:] += db / B
    out = {key: np.stack(v, axis=1) for key, v in rows.items()}
    out["value"] = val
    return out, acc
