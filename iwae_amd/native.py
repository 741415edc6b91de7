"""NativeModel: numpy-in / numpy-out wrapper over the C ABI (include/iwae_amd.h).

This is the layer the reference-API shims (iwae1.py, iwae2.py, task02.py) delegate to.
All compute happens in libiwae_amd.so on the GPU; nothing here falls back to the CPU.
"""
import ctypes as C
import numpy as np

from . import _capi
from ._capi import (AIS_INITS, IMPUTE_OUTPUT_FIELDS, LOCAL_OBJECTIVES, OBJECTIVES, POSTERIOR_OUTPUT_FIELDS, PRECISIONS, AisOptions, AisOutputs, Config, ImputeOptions,
                    ImputeOutputs, LocalOptions, LocalOutputs, PosteriorOptions, PosteriorOutputs, Scalars, Tensors, check)

_SCALAR_NAMES = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14", "inference_loss",
                 "mean_lpxz", "mean_lpz", "mean_lqzx", "mean_kl")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def ais_schedule(n_temps, schedule="sigmoid", delta=4.0):
    """The T + 1 = n_temps + 1 inverse temperatures of an annealing run, float32, from 0 to 1.  "sigmoid": Wu et al. 2017 (section 3.1),
    beta_t = (s_t - s_0) / (s_T - s_0) with s_t = sigmoid(delta (2 t / T - 1)), delta = 4: more temperatures near both ends; "linear":
    t / T.  Pure host code (no GPU)."""
    T = int(n_temps)
    if T < 1:
        raise ValueError("ais_schedule: n_temps must be at least 1")
    t = np.arange(T + 1, dtype=np.float64)
    if schedule == "linear":
        b = t / T
    elif schedule == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-float(delta) * (2.0 * t / T - 1.0)))
        b = (s - s[0]) / (s[-1] - s[0])
    else:
        raise ValueError("ais_schedule: schedule must be 'sigmoid' or 'linear', got %r" % (schedule,))
    b = np.clip(b, 0.0, 1.0)
    b[0], b[-1] = 0.0, 1.0
    return b.astype(np.float32)


class NativeModel:
    def __init__(self, n_layers, n_hidden, n_latent, x_dim=784, device=0, seed=123, world_size=1, rank=0, cond_dim=0, cond_prior=False, precision="bf16",
                 options=None):
        self.lib = _capi.load()
        cfg = Config()
        cfg.n_layers = int(n_layers)
        nh = list(n_hidden) if isinstance(n_hidden, (list, tuple)) else [n_hidden]
        nl = list(n_latent) if isinstance(n_latent, (list, tuple)) else [n_latent]
        for i in range(2):
            cfg.n_hidden[i] = int(nh[i]) if i < len(nh) else 0
            cfg.n_latent[i] = int(nl[i]) if i < len(nl) else 0
        cfg.x_dim, cfg.device, cfg.seed = int(x_dim), int(device), int(seed)
        cfg.world_size, cfg.rank = int(world_size), int(rank)
        cfg.cond_dim = int(cond_dim)
        cfg.cond_prior = 1 if cond_prior else 0
        cfg.precision = PRECISIONS[precision]
        self.precision = precision
        self.cond_dim = int(cond_dim)
        self.n_layers, self.x_dim = cfg.n_layers, cfg.x_dim
        self.n_hidden, self.n_latent = nh[:cfg.n_layers], nl[:cfg.n_layers]
        h = C.c_void_p()
        check(self.lib.iwae_create(C.byref(cfg), C.byref(h)))
        self.h = h
        n = C.c_size_t()
        check(self.lib.iwae_param_count(self.h, C.byref(n)))
        self.n_params = n.value
        for name, value in (options or {}).items():      # kernel-selection switches (A/B measurements, variant tests): iwae_set_option
            self.set_option(name, value)

    def set_option(self, name, value=1):
        check(self.lib.iwae_set_option(self.h, str(name).encode(), int(value)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.iwae_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------------------
    def tensor_table(self):
        n = C.c_int32()
        check(self.lib.iwae_num_tensors(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            name = C.create_string_buffer(64)
            r, c, off = C.c_int32(), C.c_int32(), C.c_size_t()
            check(self.lib.iwae_tensor_info(self.h, i, name, 64, C.byref(r), C.byref(c), C.byref(off)))
            shape = (r.value,) if name.value.endswith(b"bias") else (r.value, c.value)
            out.append((name.value.decode(), shape, off.value))
        return out

    def get_params(self):
        a = np.empty(self.n_params, dtype=np.float32)
        check(self.lib.iwae_get_params(self.h, a.ctypes.data, a.size))
        return a

    def set_params(self, flat):
        a = _f32(flat).ravel()
        check(self.lib.iwae_set_params(self.h, a.ctypes.data, a.size))

    def set_output_bias(self, bias):
        a = _f32(bias).ravel()
        check(self.lib.iwae_set_output_bias(self.h, a.ctypes.data, a.size))

    def get_grads(self):
        a = np.empty(self.n_params, dtype=np.float32)
        check(self.lib.iwae_get_grads(self.h, a.ctypes.data, a.size))
        return a

    def get_adam_state(self):
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        t = C.c_int64()
        check(self.lib.iwae_get_adam_state(self.h, m.ctypes.data, v.ctypes.data, m.size, C.byref(t)))
        return m, v, t.value

    def set_adam_state(self, m, v, t):
        m, v = _f32(m).ravel(), _f32(v).ravel()
        check(self.lib.iwae_set_adam_state(self.h, m.ctypes.data, v.ctypes.data, m.size, int(t)))

    def grad_devptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.iwae_grad_devptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_stream(self, stream_ptr):
        check(self.lib.iwae_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_condition(self, y):
        """Conditional model (cond_dim > 0): y [n, cond_dim] float32 for the next forward / train step / eval_llh / decode."""
        y = _f32(y).reshape(-1, self.cond_dim)
        check(self.lib.iwae_set_condition(self.h, y.ctypes.data, y.shape[0]))

    # ---- data-parallel training inside the library (RCCL) -------------------------------
    @staticmethod
    def comm_unique_id():
        """Rank 0: the opaque id blob every rank passes to comm_init (ship it with any channel)."""
        lib = _capi.load()
        buf = C.create_string_buffer(1024)
        n = C.c_size_t()
        check(lib.iwae_comm_unique_id(buf, 1024, C.byref(n)))
        return buf.raw[:n.value]

    def comm_init(self, unique_id, world_size, rank):
        """Collective over all ranks: from now on train_step all-reduces the gradient inside the library."""
        blob = bytes(unique_id)
        check(self.lib.iwae_comm_init(self.h, blob, len(blob), int(world_size), int(rank)))
        self.comm = True

    def comm_preflight(self, unique_id, world_size, rank):
        """The non-collective checks of comm_init (arguments, state, RCCL loadable); raises like comm_init would, without the rendezvous."""
        blob = bytes(unique_id)
        check(self.lib.iwae_comm_preflight(self.h, blob, len(blob), int(world_size), int(rank)))

    def comm_info(self):
        """(world size, rank) as RCCL reports them for the handle's communicators; (0, -1) without communicators."""
        w, r = C.c_int32(), C.c_int32()
        check(self.lib.iwae_comm_info(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def comm_destroy(self):
        check(self.lib.iwae_comm_destroy(self.h))
        self.comm = False

    def set_step(self, noise_step, batch_offset=0):
        check(self.lib.iwae_set_step(self.h, int(noise_step), int(batch_offset)))

    def sync(self):
        check(self.lib.iwae_sync(self.h))

    # ---- calls ------------------------------------------------------------------------
    def _eps_arg(self, eps, B, k):
        if eps is None:
            return None, None
        if self.n_layers == 1:
            e = _f32(eps)
            assert e.shape == (k, B, self.n_latent[0]), e.shape
            return e, e.ctypes.data
        e1, e2 = _f32(eps[0]), _f32(eps[1])
        assert e1.shape == (k, B, self.n_latent[0]) and e2.shape == (k, B, self.n_latent[1])
        e = np.concatenate([e1.ravel(), e2.ravel()])
        return e, e.ctypes.data

    def _want(self, want, B, k):
        if not want:
            return None, {}
        t = Tensors()
        D1 = self.n_latent[0]
        D2 = self.n_latent[1] if self.n_layers == 2 else 0
        shapes = {"z": (k, B, D1), "z2": (k, B, D2), "snis_z": (B, D1), "snis_z2": (B, D2), "al": (k, B),
                  "logits": (k, B, self.x_dim), "lpxz": (k, B), "lpz": (k, B), "lqzx": (k, B), "lpz2": (k, B),
                  "lqzx2": (k, B), "log_w": (k, B)}
        bufs = {}
        for name in want:
            if name in ("z2", "snis_z2", "lpz2", "lqzx2") and self.n_layers == 1:
                continue
            bufs[name] = np.empty(shapes[name], dtype=np.float32)
            setattr(t, name, bufs[name].ctypes.data)
        return t, bufs

    def _mask_arg(self, who, mask, x):
        """The [B, x_dim] uint8 mask of a masked call (non-zero = observed), kept alive by the caller for the call's duration."""
        mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1, self.x_dim)
        if x.ndim != 2 or mk.shape != x.shape:
            raise ValueError("%s: mask must be [B, x_dim] = %s, got %s" % (who, x.shape, mk.shape))
        return mk

    @staticmethod
    def _scalars_dict(s):
        return {n: float(getattr(s, n)) for n in _SCALAR_NAMES}

    def forward(self, x, k, beta=1.0, eps=None, want=(), mask=None):
        """mask [B, x_dim], non-zero = observed (iwae_forward_masked: the 1-layer unconditional model; float32 handles of every width, bf16
        handles whose hidden width pads to 64, 128 or 224 -- the two precisions compute different numbers: bf16 operands against float32);
        None: every pixel."""
        x = _f32(x)
        B = x.shape[0]
        keep, ep = self._eps_arg(eps, B, k)
        t, bufs = self._want(want, B, k)
        s = Scalars()
        if mask is not None:
            mk = self._mask_arg("forward", mask, x)
            check(self.lib.iwae_forward_masked(self.h, x.ctypes.data, mk.ctypes.data, B, int(k), float(beta), ep, C.byref(s),
                                               C.byref(t) if t is not None else None))
        else:
            check(self.lib.iwae_forward(self.h, x.ctypes.data, B, int(k), float(beta), ep, C.byref(s),
                                        C.byref(t) if t is not None else None))
        out = self._scalars_dict(s)
        out.update(bufs)
        return out

    def forward_backward(self, x, k, beta=1.0, objective="iwae_elbo", eps=None, want=(), mask=None):
        x = _f32(x)
        B = x.shape[0]
        keep, ep = self._eps_arg(eps, B, k)
        t, bufs = self._want(want, B, k)
        s = Scalars()
        if mask is not None:      # (iwae_forward_backward_masked: as forward)
            mk = self._mask_arg("forward_backward", mask, x)
            check(self.lib.iwae_forward_backward_masked(self.h, x.ctypes.data, mk.ctypes.data, B, int(k), float(beta), OBJECTIVES[objective], ep,
                                                        C.byref(s), C.byref(t) if t is not None else None))
        else:
            check(self.lib.iwae_forward_backward(self.h, x.ctypes.data, B, int(k), float(beta), OBJECTIVES[objective], ep,
                                                 C.byref(s), C.byref(t) if t is not None else None))
        out = self._scalars_dict(s)
        out.update(bufs)
        return out

    def set_adam(self, beta_1=0.9, beta_2=0.999, epsilon=1e-4):
        """keras.optimizers.Adam hyper-parameters of the device optimizer (default: the reference's, main.py:93)."""
        check(self.lib.iwae_set_adam(self.h, float(beta_1), float(beta_2), float(epsilon)))

    def set_eval_precision(self, precision):
        """Arithmetic of eval_llh: "fp32" (default, the reference's) or "bf16" (the fast path)."""
        check(self.lib.iwae_set_eval_precision(self.h, PRECISIONS[precision]))

    def adam_step(self, lr, grad_scale=1.0):
        check(self.lib.iwae_adam_step(self.h, float(lr), float(grad_scale)))

    def train_step(self, x, k, beta=1.0, lr=1e-3, objective="iwae_elbo", eps=None, want=(), scalars=True, mask=None):
        x = _f32(x)
        B = x.shape[0]
        keep, ep = self._eps_arg(eps, B, k)
        t, bufs = self._want(want, B, k)
        s = Scalars()
        if mask is not None:      # (iwae_train_step_masked: as forward)
            mk = self._mask_arg("train_step", mask, x)
            check(self.lib.iwae_train_step_masked(self.h, x.ctypes.data, mk.ctypes.data, B, int(k), float(beta), float(lr), OBJECTIVES[objective], ep,
                                                  C.byref(s) if scalars else None, C.byref(t) if t is not None else None))
        else:
            check(self.lib.iwae_train_step(self.h, x.ctypes.data, B, int(k), float(beta), float(lr), OBJECTIVES[objective], ep,
                                           C.byref(s) if scalars else None, C.byref(t) if t is not None else None))
        out = self._scalars_dict(s) if scalars else {}
        out.update(bufs)
        return out

    def train_step_devptr(self, x_devptr, B, k, beta, lr, objective_id):
        """Hot loop entry for benchmarks: x already resident in HBM, no host round trip."""
        check(self.lib.iwae_train_step(self.h, C.c_void_p(x_devptr), int(B), int(k), float(beta), float(lr), int(objective_id),
                                       None, None, None))

    def train_step_masked_devptr(self, x_devptr, mask_devptr, B, k, beta, lr, objective_id):
        """train_step_devptr with a resident uint8 mask [B, x_dim] (iwae_train_step_masked)."""
        check(self.lib.iwae_train_step_masked(self.h, C.c_void_p(x_devptr), C.c_void_p(mask_devptr), int(B), int(k), float(beta), float(lr),
                                              int(objective_id), None, None, None))

    def forward_backward_devptr(self, x_devptr, B, k, beta, objective_id):
        check(self.lib.iwae_forward_backward(self.h, C.c_void_p(x_devptr), int(B), int(k), float(beta), int(objective_id),
                                             None, None, None))

    def forward_backward_split_devptr(self, x_devptr, B, k, beta, objective_id):
        """iwae_forward_backward_split: returns (side stream handle, first float of the gradient segment completed on it)."""
        side, off = C.c_void_p(), C.c_size_t()
        check(self.lib.iwae_forward_backward_split(self.h, C.c_void_p(x_devptr), int(B), int(k), float(beta), int(objective_id),
                                                   None, C.byref(side), C.byref(off)))
        return side.value or 0, off.value

    def eval_llh(self, x, k=5000, chunk=0, per_image=False):
        x = _f32(x)
        N = x.shape[0]
        llh = C.c_double()
        pi = np.empty(N, dtype=np.float32) if per_image else None
        check(self.lib.iwae_eval_llh(self.h, x.ctypes.data, N, int(k), int(chunk), C.byref(llh),
                                     pi.ctypes.data if per_image else None))
        return (llh.value, pi) if per_image else llh.value

    def decode(self, z):
        z = _f32(z)
        out = np.empty((z.shape[0], self.x_dim), dtype=np.float32)
        check(self.lib.iwae_decode(self.h, z.ctypes.data, z.shape[0], out.ctypes.data))
        return out

    def grid_posterior(self, x, z, log_wq=None, log_joint=False):
        """iwae_grid_posterior: the true posterior p(z|x) and log p(x) of each image on the grid z [G, D] with log quadrature weights
        log_wq [G] (None: 0).  Returns log_px [N] (float64), post_mean [N, D], post_cov [N, D, D], q_mu, q_sigma [N, D], q_mass [N],
        kl_q_post [N] and, with log_joint=True, log_joint [N, G] = log p(x|z_g) + log p(z_g)."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D = x.shape[0], self.n_latent[0]
        z = _f32(z)
        if z.ndim == 1 and D == 1:
            z = z.reshape(-1, 1)
        if z.ndim != 2 or z.shape[1] != D:
            raise ValueError("grid_posterior: z must be [G, %d] (the latent width), got %s" % (D, z.shape))
        G = z.shape[0]
        lw = None
        if log_wq is not None:
            lw = _f32(log_wq).ravel()
            if lw.size != G:
                raise ValueError("grid_posterior: log_wq must have one entry per grid point (%d), got %d" % (G, lw.size))
        out = {"log_px": np.empty(N, dtype=np.float64), "post_mean": np.empty((N, D), dtype=np.float32),
               "post_cov": np.empty((N, D, D), dtype=np.float32), "q_mu": np.empty((N, D), dtype=np.float32),
               "q_sigma": np.empty((N, D), dtype=np.float32), "q_mass": np.empty(N, dtype=np.float32),
               "kl_q_post": np.empty(N, dtype=np.float32)}
        if log_joint:
            out["log_joint"] = np.empty((N, G), dtype=np.float32)
        ptrs = [out[k].ctypes.data for k in ("log_px", "post_mean", "post_cov", "q_mu", "q_sigma", "q_mass", "kl_q_post")]
        check(self.lib.iwae_grid_posterior(self.h, x.ctypes.data, N, z.ctypes.data, lw.ctypes.data if lw is not None else None, G, *ptrs,
                                           out["log_joint"].ctypes.data if log_joint else None))
        return out

    def latent_activity(self, x, k=5000, eps=None, per_image=False):
        """iwae_latent_activity: the activity A_u = Cov_x(E_q[u|x]) of every latent unit over the images x [N, x_dim] (Burda et al.
        section 5.2).  Layer 1: E_q[z1|x] = mu1(x); layer 2 (2-layer model): the mean of mu2(z1) over k draws of z1 ~ q(z1|x), the
        device's (eps=None) or eps [k, N, D1].  Returns {"activity": [A per layer], "data_mean": [mean over x per layer]} (float64)
        and, with per_image=True, "post_mean": [[N, D_l] per layer] (float32)."""
        x = _f32(x).reshape(-1, self.x_dim)
        N = x.shape[0]
        dims = list(self.n_latent)
        Dt = sum(dims)
        e = None
        if eps is not None and self.n_layers == 2:
            e = _f32(eps)
            if e.shape != (int(k), N, dims[0]):
                raise ValueError("latent_activity: eps must be [k, N, %d] = %s, got %s" % (dims[0], (int(k), N, dims[0]), e.shape))
        act = np.empty(Dt, dtype=np.float64)
        dm = np.empty(Dt, dtype=np.float64)
        pm = np.empty((N, Dt), dtype=np.float32) if per_image else None
        check(self.lib.iwae_latent_activity(self.h, x.ctypes.data, N, int(k), e.ctypes.data if e is not None else None,
                                            act.ctypes.data_as(C.POINTER(C.c_double)), dm.ctypes.data_as(C.POINTER(C.c_double)),
                                            pm.ctypes.data if per_image else None))
        cut = np.cumsum([0] + dims)
        out = {"activity": [act[cut[i]:cut[i + 1]] for i in range(len(dims))], "data_mean": [dm[cut[i]:cut[i + 1]] for i in range(len(dims))]}
        if per_image:
            out["post_mean"] = [np.ascontiguousarray(pm[:, cut[i]:cut[i + 1]]) for i in range(len(dims))]
        return out

    def aggregate_posterior(self, x, n_samples=1, eps=None, per_sample=False):
        """iwae_aggregate_posterior: the split of the mean KL(q(z|x_n) || p(z)) over the images x [N, x_dim] into mi = I_q(n; z),
        tc = KL(q(z) || prod_d q(z_d)) and dim_kl = sum_d KL(q(z_d) || p(z_d)), q(z) the mixture of all N encoder posteriors, from
        n_samples draws per image: the device's (eps=None; advances the noise step) or eps [n_samples, N, D].  Returns float64 scalars
        mi, tc, dim_kl, kl, log_n, arrays unit_kl, unit_mi [D] (float64) and q_mu, q_sigma [N, D]; with per_sample=True also log_qz
        [n_samples, N] and log_qzd [n_samples, N, D]."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D, S = x.shape[0], self.n_latent[0], int(n_samples)
        e = None
        if eps is not None:
            e = _f32(eps)
            if e.shape != (S, N, D):
                raise ValueError("aggregate_posterior: eps must be [n_samples, N, %d] = %s, got %s" % (D, (S, N, D), e.shape))
        summary = np.empty(4, dtype=np.float64)
        ukl, umi = np.empty(D, dtype=np.float64), np.empty(D, dtype=np.float64)
        qmu, qsg = np.empty((N, D), dtype=np.float32), np.empty((N, D), dtype=np.float32)
        lqz = np.empty((max(S, 0), N), dtype=np.float32) if per_sample else None
        lqzd = np.empty((max(S, 0), N, D), dtype=np.float32) if per_sample else None
        dp = C.POINTER(C.c_double)
        check(self.lib.iwae_aggregate_posterior(self.h, x.ctypes.data, N, S, e.ctypes.data if e is not None else None,
                                                summary.ctypes.data_as(dp), ukl.ctypes.data_as(dp), umi.ctypes.data_as(dp),
                                                qmu.ctypes.data, qsg.ctypes.data,
                                                lqz.ctypes.data if per_sample else None, lqzd.ctypes.data if per_sample else None))
        out = {"mi": summary[0], "tc": summary[1], "dim_kl": summary[2], "kl": summary[3], "log_n": np.float64(np.log(N)),
               "unit_kl": ukl, "unit_mi": umi, "q_mu": qmu, "q_sigma": qsg}
        if per_sample:
            out["log_qz"], out["log_qzd"] = lqz, lqzd
        return out

    def _mask_of(self, who, mask, x):
        """mask as the uint8 [N, x_dim] array the masked analyses take (non-zero = observed)"""
        mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1, self.x_dim)
        if mk.shape != x.shape:
            raise ValueError("%s: mask must be [N, x_dim] = %s, got %s" % (who, x.shape, mk.shape))
        return mk

    def ais(self, x, n_chains=16, n_temps=1000, leapfrog=10, step_size=0.1, adapt=True, init="encoder", betas=None, z0=None, noise=None,
            trace=False, schedule="sigmoid", mask=None):
        """iwae_ais: annealed importance sampling log p(x) of the images x [N, x_dim] with n_chains HMC chains each through the
        temperatures betas [T + 1] (default: ais_schedule(n_temps, schedule)); init "encoder" (q(z|x)) or "prior" (N(0, I)); z0 [C, N, D]
        starts the chains there (the reverse run of bidirectional Monte Carlo); noise = (eps0 [C, N, D], mom [T, C, N, D], unif [T, C, N])
        replaces the device generator.  Returns log_px [N] and log_w [C, N] (float64), ess [N], accept_rate [T], z [C, N, D] (final
        states), step_size [C, N], q_mu, q_sigma [N, D], betas; with trace=True also dH [T, C, N] and accepted [T, C, N] (uint8).
        mask [N, x_dim] (non-zero = observed; iwae_ais_masked): the images are incomplete, log_px estimates log p(x_obs), the chains target
        p(z | x_obs) and the encoder sees mask ? x : 0; what x holds at an unobserved pixel is never read."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D, Cn = x.shape[0], self.n_latent[0], int(n_chains)
        b = ais_schedule(n_temps, schedule) if betas is None else _f32(betas).ravel()
        T = b.size - 1
        o = AisOptions()
        o.C, o.T, o.L = Cn, T, int(leapfrog)
        o.betas = b.ctypes.data
        o.step_size, o.adapt = float(step_size), 1 if adapt else 0
        if init not in AIS_INITS:
            raise ValueError("ais: init must be 'encoder' or 'prior', got %r" % (init,))
        o.init = AIS_INITS[init]
        keep = [b]
        if z0 is not None:
            z0 = _f32(z0)
            if z0.shape != (Cn, N, D):
                raise ValueError("ais: z0 must be [n_chains, N, %d] = %s, got %s" % (D, (Cn, N, D), z0.shape))
            o.z0 = z0.ctypes.data
        if noise is not None:
            e0, mom, unif = (_f32(v) for v in noise)
            if e0.shape != (Cn, N, D) or mom.shape != (T, Cn, N, D) or unif.shape != (T, Cn, N):
                raise ValueError("ais: noise must be (eps0 %s, mom %s, unif %s), got %s, %s, %s"
                                 % ((Cn, N, D), (T, Cn, N, D), (T, Cn, N), e0.shape, mom.shape, unif.shape))
            o.eps0, o.mom, o.unif = e0.ctypes.data, mom.ctypes.data, unif.ctypes.data
            keep += [e0, mom, unif]
        n0, c0, t0 = max(N, 0), max(Cn, 0), max(T, 0)      # (bad counts: the library rejects them; nothing is written)
        res = {"log_px": np.empty(n0, dtype=np.float64), "log_w": np.empty((c0, n0), dtype=np.float64), "ess": np.empty(n0, dtype=np.float32),
               "accept_rate": np.empty(t0, dtype=np.float32), "z": np.empty((c0, n0, D), dtype=np.float32),
               "step_out": np.empty((c0, n0), dtype=np.float32), "q_mu": np.empty((n0, D), dtype=np.float32),
               "q_sigma": np.empty((n0, D), dtype=np.float32)}
        if trace:
            res["dH"] = np.empty((t0, c0, n0), dtype=np.float32)
            res["accepted"] = np.empty((t0, c0, n0), dtype=np.uint8)
        outs = AisOutputs()
        for name, arr in res.items():
            setattr(outs, name, arr.ctypes.data)
        if mask is None:
            check(self.lib.iwae_ais(self.h, x.ctypes.data, N, C.byref(o), C.byref(outs)))
        else:
            mk = self._mask_of("ais", mask, x)
            check(self.lib.iwae_ais_masked(self.h, x.ctypes.data, mk.ctypes.data, N, C.byref(o), C.byref(outs)))
        res["step_size"] = res.pop("step_out")
        res["betas"] = b
        return res

    def local_posterior(self, x, n_samples=16, n_iters=200, n_eval=8, objective="elbo", lr=0.05, start=None, noise=None, trace=False,
                        beta_1=0.9, beta_2=0.999, epsilon=1e-4, mask=None):
        """iwae_local_posterior: a factorised Gaussian q per image of x [N, x_dim], moved by n_iters Adam iterations that ascend the
        n_samples-draw bound `objective` ("elbo" or "iwae") from start = (mu0, sigma0) [N, D] each (None: the encoder heads), then scored
        on n_eval passes of n_samples fresh draws.  noise [n_iters + n_eval, n_samples, N, D] replaces the device generator (and leaves
        the noise step alone).  Returns elbo, iwae [N] (float64), mu, sigma (optimised), q_mu, q_sigma (the start) [N, D], log_w
        [n_eval n_samples, N]; with trace=True also bound [n_iters, N] and grad [N, 2 D] (the last iteration's; absent at n_iters = 0).
        mask [N, x_dim] (non-zero = observed; iwae_local_posterior_masked): q is fitted to p(z | x_obs), the encoder start is the heads of
        mask ? x : 0, and what x holds at an unobserved pixel is never read."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D, S, T, E = x.shape[0], self.n_latent[0], int(n_samples), int(n_iters), int(n_eval)
        if objective not in LOCAL_OBJECTIVES:
            raise ValueError("local_posterior: objective must be 'elbo' or 'iwae', got %r" % (objective,))
        o = LocalOptions()
        o.S, o.T, o.E, o.objective = S, T, E, LOCAL_OBJECTIVES[objective]
        o.lr, o.beta_1, o.beta_2, o.epsilon = float(lr), float(beta_1), float(beta_2), float(epsilon)
        keep = []
        if start is not None:
            mu0, sg0 = (_f32(v) for v in start)
            if mu0.shape != (N, D) or sg0.shape != (N, D):
                raise ValueError("local_posterior: start must be (mu0, sigma0) of shape %s each, got %s, %s" % ((N, D), mu0.shape, sg0.shape))
            o.mu0, o.sigma0 = mu0.ctypes.data, sg0.ctypes.data
            keep += [mu0, sg0]
        n0, s0, t0, e0 = max(N, 0), max(S, 0), max(T, 0), max(E, 0)      # (bad counts: the library rejects them; nothing is written)
        if noise is not None:
            e = _f32(noise)
            if e.shape != (t0 + e0, s0, n0, D):
                raise ValueError("local_posterior: noise must be [n_iters + n_eval, n_samples, N, %d] = %s, got %s" % (D, (t0 + e0, s0, n0, D), e.shape))
            o.eps = e.ctypes.data
            keep.append(e)
        res = {"elbo": np.empty(n0, dtype=np.float64), "iwae": np.empty(n0, dtype=np.float64)}
        for name in ("mu", "sigma", "q_mu", "q_sigma"):
            res[name] = np.empty((n0, D), dtype=np.float32)
        res["log_w"] = np.empty((e0 * s0, n0), dtype=np.float32)
        if trace:
            res["bound"] = np.empty((t0, n0), dtype=np.float32)
            if t0 > 0:
                res["grad"] = np.empty((n0, 2 * D), dtype=np.float32)
        outs = LocalOutputs()
        for name, arr in res.items():
            setattr(outs, name, arr.ctypes.data)
        if mask is None:
            check(self.lib.iwae_local_posterior(self.h, x.ctypes.data, N, C.byref(o), C.byref(outs)))
        else:
            mk = self._mask_of("local_posterior", mask, x)
            check(self.lib.iwae_local_posterior_masked(self.h, x.ctypes.data, mk.ctypes.data, N, C.byref(o), C.byref(outs)))
        return res

    def impute(self, x, mask=None, n_samples=50, noise=None, outputs=IMPUTE_OUTPUT_FIELDS):
        """iwae_impute: the n_samples-draw importance-weighted bound on log p(x_obs) of the images x [N, x_dim] whose observed pixels mask
        [N, x_dim] marks (non-zero; None: every pixel observed), and the self-normalised estimate xhat = sum_s al_s sigmoid(l_s) of
        E[x | x_obs] at every pixel.  What x holds at an unobserved pixel is never read.  noise [n_samples, N, D] replaces the device
        generator (and leaves the noise step alone).  outputs: which of log_px [N] (float64; always), xhat [N, x_dim], ess [N], log_w
        [n_samples, N], q_mu, q_sigma [N, D] to return (xhat left out: the second decoder pass does not run).  Returns a dict."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D, S = x.shape[0], self.n_latent[0], int(n_samples)
        unknown = set(outputs) - set(IMPUTE_OUTPUT_FIELDS)
        if unknown:
            raise ValueError("impute: unknown outputs %s (known: %s)" % (sorted(unknown), ", ".join(IMPUTE_OUTPUT_FIELDS)))
        o = ImputeOptions()
        o.k = S
        keep = []
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1, self.x_dim)
            if mk.shape != x.shape:
                raise ValueError("impute: mask must be [N, x_dim] = %s, got %s" % (x.shape, mk.shape))
            o.mask = mk.ctypes.data
            keep.append(mk)
        n0, s0 = max(N, 0), max(S, 0)      # (bad counts: the library rejects them; nothing is written)
        if noise is not None:
            e = _f32(noise)
            if e.shape != (s0, n0, D):
                raise ValueError("impute: noise must be [n_samples, N, %d] = %s, got %s" % (D, (s0, n0, D), e.shape))
            o.eps = e.ctypes.data
            keep.append(e)
        shapes = {"log_px": ((n0,), np.float64), "xhat": ((n0, self.x_dim), np.float32), "ess": ((n0,), np.float32),
                  "log_w": ((s0, n0), np.float32), "q_mu": ((n0, D), np.float32), "q_sigma": ((n0, D), np.float32)}
        res = {name: np.empty(*shapes[name]) for name in IMPUTE_OUTPUT_FIELDS if name == "log_px" or name in outputs}
        outs = ImputeOutputs()
        for name, arr in res.items():
            setattr(outs, name, arr.ctypes.data)
        check(self.lib.iwae_impute(self.h, x.ctypes.data, N, C.byref(o), C.byref(outs)))
        return res

    def posterior(self, x, mask=None, n_samples=5000, n_draws=0, noise=None, uniforms=None, outputs=None):
        """iwae_posterior: on the n_samples importance draws iwae_impute would take for the images x [N, x_dim] (mask, noise: as impute),
        the self-normalised estimates mean [N, D] and cov [N, D, D] of the posterior p(z | x_obs), and n_draws latent vectors per image
        resampled from it with replacement (SIR): idx [n_draws, N] (int32, into the proposals), z [n_draws, N, D], u [n_draws, N] the
        uniforms used.  uniforms [n_draws, N] replaces the device generator; u_r = (r + u0) / n_draws gives systematic resampling.  The
        noise step advances by one unless everything drawn was the caller's.  outputs: which of log_px [N] (float64; always), ess, mean,
        cov, idx, z, u, log_w [n_samples, N], q_mu, q_sigma to return (None: all, idx / z / u only when n_draws > 0).  Returns a dict."""
        x = _f32(x).reshape(-1, self.x_dim)
        N, D, S, R = x.shape[0], self.n_latent[0], int(n_samples), int(n_draws)
        if outputs is None:
            outputs = tuple(f for f in POSTERIOR_OUTPUT_FIELDS if R > 0 or f not in ("idx", "z", "u"))
        unknown = set(outputs) - set(POSTERIOR_OUTPUT_FIELDS)
        if unknown:
            raise ValueError("posterior: unknown outputs %s (known: %s)" % (sorted(unknown), ", ".join(POSTERIOR_OUTPUT_FIELDS)))
        o = PosteriorOptions()
        o.k, o.R = S, R
        keep = []
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1, self.x_dim)
            if mk.shape != x.shape:
                raise ValueError("posterior: mask must be [N, x_dim] = %s, got %s" % (x.shape, mk.shape))
            o.mask = mk.ctypes.data
            keep.append(mk)
        n0, s0, r0 = max(N, 0), max(S, 0), max(R, 0)      # (bad counts: the library rejects them; nothing is written)
        if noise is not None:
            e = _f32(noise)
            if e.shape != (s0, n0, D):
                raise ValueError("posterior: noise must be [n_samples, N, %d] = %s, got %s" % (D, (s0, n0, D), e.shape))
            o.eps = e.ctypes.data
            keep.append(e)
        if uniforms is not None:
            un = _f32(uniforms)
            if un.shape != (r0, n0):
                raise ValueError("posterior: uniforms must be [n_draws, N] = %s, got %s" % ((r0, n0), un.shape))
            o.unif = un.ctypes.data
            keep.append(un)
        shapes = {"log_px": ((n0,), np.float64), "ess": ((n0,), np.float32), "mean": ((n0, D), np.float32), "cov": ((n0, D, D), np.float32),
                  "idx": ((r0, n0), np.int32), "z": ((r0, n0, D), np.float32), "u": ((r0, n0), np.float32),
                  "log_w": ((s0, n0), np.float32), "q_mu": ((n0, D), np.float32), "q_sigma": ((n0, D), np.float32)}
        res = {name: np.empty(*shapes[name]) for name in POSTERIOR_OUTPUT_FIELDS if name == "log_px" or name in outputs}
        outs = PosteriorOutputs()
        for name, arr in res.items():
            setattr(outs, name, arr.ctypes.data)
        check(self.lib.iwae_posterior(self.h, x.ctypes.data, N, C.byref(o), C.byref(outs)))
        return res

    def grad_moments(self, x, k, draws, beta=1.0, objective="iwae_elbo"):
        """iwae_grad_moments: the per-parameter mean and unbiased variance (float64 [P] each) of `draws` gradient draws of the training
        estimator on the images x [B, x_dim].  Draw j is the gradient forward_backward(x, k, beta, objective) leaves after
        set_step(s0 + j), s0 the current step; the step advances by `draws`, parameters and Adam state stay as they are."""
        x = _f32(x).reshape(-1, self.x_dim)
        mean = np.empty(self.n_params, dtype=np.float64)
        var = np.empty(self.n_params, dtype=np.float64)
        check(self.lib.iwae_grad_moments(self.h, x.ctypes.data, x.shape[0], int(k), float(beta), OBJECTIVES[objective], int(draws),
                                         mean.ctypes.data_as(C.POINTER(C.c_double)), var.ctypes.data_as(C.POINTER(C.c_double))))
        return mean, var

    def grad_moments_devptr(self, x_ptr, B, k, draws, beta, objective_id, mean_ptr, var_ptr):
        """iwae_grad_moments on raw pointers (host or device: x [B, x_dim] float32, mean / var [P] float64)."""
        check(self.lib.iwae_grad_moments(self.h, C.c_void_p(x_ptr), int(B), int(k), float(beta), int(objective_id), int(draws),
                                         C.cast(C.c_void_p(mean_ptr), C.POINTER(C.c_double)), C.cast(C.c_void_p(var_ptr), C.POINTER(C.c_double))))

    # ---- resident dataset (device-side shuffle order + dynamic binarisation) -------------------
    def dataset_upload(self, gray_u8):
        g = np.ascontiguousarray(gray_u8, dtype=np.uint8).reshape(-1, self.x_dim)
        check(self.lib.iwae_dataset_upload(self.h, g.ctypes.data, g.shape[0]))
        self.n_data = g.shape[0]

    def dataset_begin_epoch(self, epoch, order=None):
        if order is None:
            check(self.lib.iwae_dataset_begin_epoch(self.h, int(epoch), None, 0))
        else:
            o = np.ascontiguousarray(order, dtype=np.int32)
            check(self.lib.iwae_dataset_begin_epoch(self.h, int(epoch), o.ctypes.data, o.size))

    def dataset_get_batch(self, start, B):
        out = np.empty((B, self.x_dim), dtype=np.float32)
        check(self.lib.iwae_dataset_get_batch(self.h, int(start), int(B), out.ctypes.data))
        return out

    def dataset_set_labels(self, labels):
        """One class id (< cond_dim) per image of the uploaded set: conditional models on the resident dataset (tasks/task05.py:296-322)."""
        y = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        check(self.lib.iwae_dataset_set_labels(self.h, y.ctypes.data, y.size))

    def dataset_get_labels(self, start, B):
        out = np.empty((B, self.cond_dim), dtype=np.float32)
        check(self.lib.iwae_dataset_get_labels(self.h, int(start), int(B), out.ctypes.data))
        return out

    def dataset_set_mask(self, mask):
        """One fixed mask per image of the uploaded set, [n, x_dim], non-zero = observed (iwae_dataset_set_mask): train_step_dataset then takes
        the masked step on (dataset_get_batch, dataset_get_mask) of its rows.  A NumPy array, or a torch uint8 tensor on the handle's device
        (packed in place); None drops the masks."""
        if mask is None:
            check(self.lib.iwae_dataset_set_mask(self.h, None, 0))
            return
        if hasattr(mask, "data_ptr") and getattr(mask, "is_cuda", False):
            if mask.dim() != 2 or mask.shape[1] != self.x_dim or mask.element_size() != 1 or not mask.is_contiguous():
                raise ValueError("dataset_set_mask: a device mask must be a contiguous [n, %d] uint8 tensor" % self.x_dim)
            check(self.lib.iwae_dataset_set_mask(self.h, C.c_void_p(mask.data_ptr()), int(mask.shape[0])))
            return
        mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1, self.x_dim)
        check(self.lib.iwae_dataset_set_mask(self.h, mk.ctypes.data, mk.shape[0]))

    def dataset_mcar_mask(self, rate, seed=0):
        """Masks drawn on the device, each pixel hidden with probability `rate` independently (iwae_dataset_mcar_mask; keyed by `seed`, not
        the handle's seed); utils.device_mcar_mask(n, x_dim, rate, seed) is the same array on the host."""
        check(self.lib.iwae_dataset_mcar_mask(self.h, float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def dataset_get_mask(self, start, B):
        """The mask rows of the batch dataset_get_batch(start, B) returns: [B, x_dim] uint8, 1 = observed."""
        out = np.empty((B, self.x_dim), dtype=np.uint8)
        check(self.lib.iwae_dataset_get_mask(self.h, int(start), int(B), out.ctypes.data))
        return out

    def train_step_dataset(self, start, B, k, beta=1.0, lr=1e-3, objective="iwae_elbo", scalars=True):
        s = Scalars()
        check(self.lib.iwae_train_step_dataset(self.h, int(start), int(B), int(k), float(beta), float(lr), OBJECTIVES[objective],
                                               C.byref(s) if scalars else None))
        return self._scalars_dict(s) if scalars else {}

    def enable_timing(self, every=1):
        """every = n > 0: bracket the dominant kernels of every n-th step with HIP events; 0 / False: off."""
        check(self.lib.iwae_enable_timing(self.h, int(every)))

    def kernel_time(self, name):
        us, cnt = C.c_double(), C.c_int64()
        check(self.lib.iwae_kernel_time(self.h, name.encode(), C.byref(us), C.byref(cnt)))
        return us.value, cnt.value

    def debug_tensor(self, name):
        r, c = C.c_int32(), C.c_int32()
        check(self.lib.iwae_debug_tensor(self.h, name.encode(), None, 0, C.byref(r), C.byref(c)))
        out = np.empty((r.value, c.value), dtype=np.float32)
        check(self.lib.iwae_debug_tensor(self.h, name.encode(), out.ctypes.data, out.size, C.byref(r), C.byref(c)))
        return out

    def debug_eps(self, B, k, layer=0):
        out = np.empty((k, B, self.n_latent[layer]), dtype=np.float32)
        check(self.lib.iwae_debug_eps(self.h, B, k, layer, out.ctypes.data))
        return out
