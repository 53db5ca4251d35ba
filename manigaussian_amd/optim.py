"""LAMB, fused: a drop-in for ManiGaussian's optimizer as two HIP launches per step for any number of tensors.

Reference: helpers/optim/lamb.py:14-111 (`Lamb`; selected by conf/method/ManiGaussian_BC.yaml:45, constructed at
agents/manigaussian_bc/qattention_manigaussian_bc_agent.py:476-483).  There `step()` is a Python loop over the parameter
tensors: about a dozen small kernels, three temporaries and two device reads per tensor (`if weight_norm == 0 or adam_norm ==
0`, and the tensor-valued alpha of the final add_).  Here (csrc/mgs_optim.hip) every gradient is a view into one flat fp32
buffer (parallel.GradBucket, or a buffer of this class), the moments live in two flat buffers, and a step is a moments pass
and an apply pass over fixed-size chunks: no host read, no allocation, deterministic, capturable into a HIP graph.
The algorithm is the reference's, quirks included: no bias correction, the weight norm clamped to [0, 10], trust ratio 1
where either norm is exactly zero, `adam=True` applies ratio 1 but records the computed one, a parameter without a gradient
is skipped entirely.
"""
import numpy as np
import torch

from . import _lib, _ops

_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("numel", "<i8"), ("state_off", "<i8"), ("group", "<i4"), ("flags", "<i4"),
                       ("chunk0", "<i4"), ("n_chunks", "<i4")])     # MgsLambTensor (include/mgsplat.h)
_GROUP_DT = np.dtype([("lr", "<f4"), ("beta1", "<f4"), ("omb1", "<f4"), ("beta2", "<f4"), ("omb2", "<f4"), ("eps", "<f4"),
                      ("wd", "<f4"), ("adam", "<i4"), ("lr_dev", "<u8")])  # MgsLambGroup
assert _TENSOR_DT.itemsize == 48 and _GROUP_DT.itemsize == 40
_P_ALIGNED, _G_ALIGNED = 1, 2


def _round4(n):
    return (n + 3) & ~3


def _up256(n):
    return (n + 255) & ~255


class FusedLamb(torch.optim.Optimizer):
    """FusedLamb(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False, *, bucket=None, grad_scale=1.0,
    zero_grad=False): the reference `Lamb`'s signature, ValueErrors, parameter groups and state-dict layout.

    Gradients: with `bucket` (a parallel.GradBucket holding every parameter) the bucket's flat buffer is read in place, behind
    its all-reduce; without, the optimizer makes its own flat buffer and points every `.grad` at its view.  A `.grad` that is
    some other tensor at step() is copied into the view and re-pointed; a `.grad` that is None skips the parameter for that step.
    grad_scale multiplies every gradient as it is read (1 / world size behind GradBucket.all_reduce, which sums);
    zero_grad=True zeroes the gradients of the parameters that stepped as they are read, replacing the separate fill.
    state[p]: `step` (int), `exp_avg` / `exp_avg_sq` (views of the flat moment buffers), `weight_norm` / `adam_norm` /
    `trust_ratio` (0-dim views of the statistics buffer: always tensors, also where the reference's ratio is the int 1).
    A group's `lr` may be a one-element float32 device tensor: the kernels then read the current value, so a step captured
    into a HIP graph follows a schedule written in place.  Python floats are copied to a device table when they changed
    (never during a capture: run one eager step first).  float32, contiguous, dense HIP tensors only; there is no CPU path."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False, *, bucket=None,
                 grad_scale=1.0, zero_grad=False):
        if not isinstance(lr, torch.Tensor) and not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.adam = adam
        self.grad_scale = float(grad_scale)
        self.fused_zero_grad = bool(zero_grad)
        self._bucket = bucket
        self._layout = None
        super().__init__(params, defaults)
        self._build()

    # ---- layout -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_param(p):
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"FusedLamb: parameters must be tensors, got {type(p).__name__}")
        if not p.is_cuda:
            raise RuntimeError(f"FusedLamb needs parameters on a HIP device; there is no CPU path (got a tensor on {p.device})")
        if p.is_sparse or p.layout != torch.strided:
            raise RuntimeError("FusedLamb does not support sparse parameters")
        if p.dtype != torch.float32:
            raise RuntimeError(f"FusedLamb: parameters must be float32, got {p.dtype}")
        if not p.is_contiguous():
            raise RuntimeError(f"FusedLamb: parameters must be contiguous, got strides {p.stride()} for shape {tuple(p.shape)}")
        if p.numel() == 0:
            raise RuntimeError("FusedLamb: empty parameter tensor")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)
        if getattr(self, "_layout", None) is not None:
            self._build()

    def _build(self):
        """Flat buffers and the chunk table for the current parameter list (moments of an earlier layout are carried over)."""
        L = _lib.lib()
        params = [p for g in self.param_groups for p in g["params"]]
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise RuntimeError("FusedLamb: every parameter must live on one device")
        old = self._layout
        chunk = L.mgs_lamb_chunk_elems()
        n = len(params)
        offs, off = [], 0
        for p in params:
            offs.append(off)
            off += _round4(p.numel())
        total = off
        f32 = dict(dtype=torch.float32, device=dev)
        # one allocation: m | v | statistics (16-byte aligned pieces)
        state = torch.zeros(2 * total + _round4(3 * n), **f32)
        m, v, stats = state[:total], state[total:2 * total], state[2 * total:2 * total + 3 * n].view(n, 3)
        if self._bucket is not None:
            by_id = {id(self._bucket.params[k]): self._bucket.views[k] for k in self._bucket.names}
            missing = [i for i, p in enumerate(params) if id(p) not in by_id]
            if missing:
                raise RuntimeError(f"FusedLamb: {len(missing)} parameter(s) are not in the GradBucket (first: index {missing[0]})")
            flat = self._bucket.flat
            views = [by_id[id(p)] for p in params]
            for p, w in zip(params, views):
                if w.shape != p.shape or w.dtype != torch.float32 or w.device != dev or not w.is_contiguous():
                    raise RuntimeError("FusedLamb: a GradBucket view does not match its parameter")
        else:
            flat = torch.zeros(total, **f32)
            views = [flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, params)]
        n_chunks = [(p.numel() + chunk - 1) // chunk for p in params]
        chunk0 = np.concatenate([[0], np.cumsum(n_chunks)]).astype(np.int64)
        total_chunks = int(chunk0[-1])
        cmap = np.empty((total_chunks, 2), dtype=np.int32)
        for i, c in enumerate(n_chunks):
            cmap[chunk0[i]:chunk0[i + 1], 0] = i
            cmap[chunk0[i]:chunk0[i + 1], 1] = np.arange(c, dtype=np.int32)
        group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        ws_bytes = L.mgs_lamb_workspace_bytes(total_chunks)
        t_bytes, g_bytes = _up256(48 * n), _up256(40 * len(self.param_groups))
        table = torch.zeros(t_bytes + g_bytes + _up256(8 * total_chunks), dtype=torch.uint8, device=dev)
        self._layout = dict(
            params=params, index={id(p): i for i, p in enumerate(params)}, dev=dev, offs=offs, total=total, state=state, m=m, v=v,
            stats=stats, flat=flat, views=views, view_ptr=[w.data_ptr() for w in views], n_chunks=n_chunks, chunk0=chunk0,
            total_chunks=total_chunks, cmap=cmap, group_of=group_of, ws=torch.empty(ws_bytes // 4, **f32), ws_bytes=ws_bytes,
            table=table, t_bytes=t_bytes, g_bytes=g_bytes, sig=None, states=[None] * n)
        if old is not None:  # moments and statistics of the parameters that were there before
            for i, p in enumerate(old["params"]):
                j = self._layout["index"].get(id(p))
                if j is None:  # (no longer a parameter of this optimizer)
                    continue
                k = p.numel()
                m[offs[j]:offs[j] + k].copy_(old["m"][old["offs"][i]:old["offs"][i] + k])
                v[offs[j]:offs[j] + k].copy_(old["v"][old["offs"][i]:old["offs"][i] + k])
                stats[j].copy_(old["stats"][i])
        for p in params:
            if p in self.state:
                self._bind_state(p, self.state[p].get("step", 0))
        for p, w in zip(params, views):  # every .grad becomes its view (a gradient that is already there keeps its values)
            g = p.grad
            if g is not None and g.data_ptr() != w.data_ptr():
                if g.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients, consider SparseAdam instad.")
                w.copy_(g)
            if g is None or g.data_ptr() != w.data_ptr():
                p.grad = w

    def _bind_state(self, p, step):
        lay = self._layout
        i = lay["index"][id(p)]
        o, k = lay["offs"][i], p.numel()
        st = dict(step=step, exp_avg=lay["m"][o:o + k].view_as(p), exp_avg_sq=lay["v"][o:o + k].view_as(p),
                  weight_norm=lay["stats"][i, 0], adam_norm=lay["stats"][i, 1], trust_ratio=lay["stats"][i, 2])
        self.state[p] = lay["states"][i] = st

    # ---- the torch.optim.Optimizer surface ---------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        """One fill of the flat gradient buffer; every `.grad` stays the view it is.  `set_to_none` is ignored: dropping the
        views would make autograd allocate fresh gradient tensors and defeat the flat buffer."""
        self._layout["flat"].zero_()

    def load_state_dict(self, state_dict):
        """Accepts the reference `Lamb`'s state dicts as well as this class's: exp_avg / exp_avg_sq are copied into the flat
        buffers, the recorded norms and ratio (tensors or Python numbers) into the statistics buffer."""
        lrs = [g["lr"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, lr in zip(self.param_groups, lrs):  # a device lr stays the tensor the caller's schedule writes to
            if isinstance(lr, torch.Tensor):
                with torch.no_grad():
                    lr.copy_(torch.as_tensor(g["lr"], dtype=torch.float32).reshape(lr.shape))
                g["lr"] = lr
        if any(id(p) not in self._layout["index"] for g in self.param_groups for p in g["params"]):
            self._build()
        lay = self._layout
        lay["states"] = [None] * len(lay["params"])
        with torch.no_grad():
            for p, st in list(self.state.items()):
                i = lay["index"][id(p)]
                o, k = lay["offs"][i], p.numel()
                lay["m"][o:o + k].copy_(st["exp_avg"].reshape(-1))
                lay["v"][o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
                for c, key in enumerate(("weight_norm", "adam_norm", "trust_ratio")):
                    val = st.get(key)
                    if isinstance(val, torch.Tensor):
                        lay["stats"][i, c].copy_(val.reshape(()))
                    elif val is not None:
                        lay["stats"][i, c].fill_(float(val))
                self._bind_state(p, int(st.get("step", 0)))
            for i, st in enumerate(lay["states"]):  # a parameter the loaded dict has no state for starts from zero moments
                if st is None:
                    o, k = lay["offs"][i], lay["params"][i].numel()
                    lay["m"][o:o + k].zero_()
                    lay["v"][o:o + k].zero_()
                    lay["stats"][i].zero_()
        lay["sig"] = None

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _signature(self):
        """What the device tables were built from: pointers and hyper-parameters, read on the host.  Also adopts foreign
        gradients (copied into the views).  -> (signature, indices of the parameters that have a gradient)."""
        lay = self._layout
        ptrs, active = [], []
        views, view_ptr = lay["views"], lay["view_ptr"]
        known = lay["sig"][0] if lay["sig"] is not None else None
        for i, p in enumerate(lay["params"]):
            g = p.grad
            pp = p.data_ptr()
            if g is None:
                ptrs.append((pp, 0))
                continue
            w = views[i]
            if g is not w and (g.data_ptr() != view_ptr[i] or g.shape != w.shape or g.dtype != torch.float32
                               or not g.is_contiguous()):
                if g.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients, consider SparseAdam instad.")
                if g.shape != w.shape or g.device != w.device:
                    raise RuntimeError(f"FusedLamb: a gradient of shape {tuple(g.shape)} on {g.device} for a parameter of "
                                       f"shape {tuple(w.shape)} on {w.device}")
                w.copy_(g)
                p.grad = w
            if known is None or known[i][0] != pp:  # a new storage (p.data replaced): is it still one this class takes?
                self._check_param(p)
                if p.shape != w.shape:
                    raise RuntimeError(f"FusedLamb: a parameter changed its shape from {tuple(w.shape)} to {tuple(p.shape)}")
            ptrs.append((pp, view_ptr[i]))
            active.append(i)
        hyper = []
        for g in self.param_groups:
            lr = g["lr"]
            if isinstance(lr, torch.Tensor):
                if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1 and lr.device == lay["dev"]):
                    raise RuntimeError("FusedLamb: a tensor lr must be one float32 element on the parameters' device")
                lr = ("dev", lr.data_ptr())
            else:
                lr = float(lr)
            hyper.append((lr, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                          bool(self.adam)))
        return (ptrs, hyper), active

    def _upload(self, sig):
        lay = self._layout
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedLamb: a pointer or a hyper-parameter changed since the last eager step; the device tables "
                               "cannot be rebuilt inside a graph capture -- run one eager step in this state first")
        ptrs, hyper = sig
        n = len(ptrs)
        tt = np.zeros(n, dtype=_TENSOR_DT)
        for i, (pp, gp) in enumerate(ptrs):
            if pp % 4 or gp % 4:
                raise RuntimeError("FusedLamb: a parameter or gradient is not 4-byte aligned")
            tt[i] = (pp, gp, lay["params"][i].numel(), lay["offs"][i], lay["group_of"][i],
                     (_P_ALIGNED if pp % 16 == 0 else 0) | (_G_ALIGNED if gp % 16 == 0 else 0), int(lay["chunk0"][i]),
                     lay["n_chunks"][i])
        gt = np.zeros(len(hyper), dtype=_GROUP_DT)
        for i, (lr, b1, b2, eps, wd, adam) in enumerate(hyper):
            dev_lr = isinstance(lr, tuple)
            # 1 - beta in double, rounded once: what torch does with the Python scalar alpha (lamb.py:82-84)
            gt[i] = (0.0 if dev_lr else lr, b1, 1 - b1, b2, 1 - b2, eps, wd, int(adam), lr[1] if dev_lr else 0)
        host = np.zeros(lay["table"].numel(), dtype=np.uint8)
        host[:tt.nbytes] = tt.view(np.uint8)
        host[lay["t_bytes"]:lay["t_bytes"] + gt.nbytes] = gt.view(np.uint8)
        cb = lay["cmap"].reshape(-1).view(np.uint8)
        host[lay["t_bytes"] + lay["g_bytes"]:lay["t_bytes"] + lay["g_bytes"] + cb.size] = cb
        # a fresh pinned block per upload (they are rare): the caching host allocator keeps it alive until the copy has run
        pinned = torch.from_numpy(host).pin_memory()
        lay["table"].copy_(pinned, non_blocking=True)
        lay["sig"] = sig

    @torch.no_grad()
    def step(self, closure=None):
        """One optimization step; returns the closure's loss like the reference."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lay = self._layout
        if len(lay["params"]) != sum(len(g["params"]) for g in self.param_groups):
            self._build()
            lay = self._layout
        sig, active = self._signature()
        if not active:
            return loss
        if sig != lay["sig"]:
            self._upload(sig)
        states = lay["states"]
        for i in active:
            st = states[i]
            if st is None:
                self._bind_state(lay["params"][i], 1)
            else:
                st["step"] += 1
        base = lay["table"].data_ptr()
        _ops.call("mgs_lamb_step", lay["dev"],
                  len(lay["params"]), len(self.param_groups), lay["total_chunks"], base, base + lay["t_bytes"],
                  base + lay["t_bytes"] + lay["g_bytes"], lay["m"].data_ptr(), lay["v"].data_ptr(), lay["stats"].data_ptr(),
                  self.grad_scale, int(self.fused_zero_grad), lay["ws"].data_ptr(), lay["ws_bytes"])
        return loss
