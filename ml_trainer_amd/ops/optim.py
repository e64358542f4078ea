"""Fused flat-buffer optimizers: SGD / Adam / AdamW / Adagrad / Adamax, and LAMB.

The reference builds one of five ``torch.optim`` optimizers by name
(``src/trainer.py:123-138``). These classes are drop-in ``torch.optim.Optimizer``
subclasses (so ``torch.optim.lr_scheduler`` works on them unchanged) whose
``step()`` is ONE HIP launch over the contiguous parameter buffer of each param
group (``csrc/kernels/optim.hip``), with the exact torch update rules
(``csrc/include/mlt_optim.h``).

State lives in flat buffers (``exp_avg`` etc. as one tensor per group) instead
of per-parameter dicts; ``state_dict()``/``load_state_dict()`` round-trip it.
On CPU tensors the same math runs as vectorised torch ops over the flat buffers
(plumbing config).

Per-tensor behaviour lives inside the one flat buffer, through a ``SegmentTable`` (tensor
boundaries, a weight decay and an "adapt" flag per tensor, cut into fixed-size chunks for the
kernels). Two optimizers use it:

* ``FusedAdamW(no_decay=[...])``: no decay on the listed parameters; one segmented launch
  (``flat_optim_seg``), per tensor bit for bit the plain launch with that tensor's decay.
* ``FusedLAMB``: layer-wise trust ratios; three launches (moments + per-chunk sums of squares,
  per-tensor norms and ratios, apply), the kernel boundaries being the grid-wide dependencies.

Torch param groups are not the way to exclude parameters here: each extra group would get a
FlatParams of its own and leave the DDP flat buffer. Both optimizers take a single group. They are
refused on a ZeRO-1 shard (shards cut tensors; a sharded norm would need a collective) and by the
fused LeNet engine (its kernels embed the five element-wise rules).
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional

import torch

from ml_trainer_amd.ops._ext import require_native
from ml_trainer_amd.utils.flat import FlatParams

KIND = {"sgd": 0, "adam": 1, "adamw": 2, "adagrad": 3, "adamax": 4, "lamb": 5}


class SegmentTable:
    """The tensors of one flat buffer, for the per-tensor optimizers (LAMB, AdamW with exclusions).

    ``segments[i] = (offset, numel)`` of ``flat.params[i]``; ``wd[i]`` its weight decay; ``adapt[i]``
    whether LAMB's trust ratio applies to it. On a device buffer the same table exists as device
    tensors, cut into chunks of at most ``_C.optim_chunk_elems()`` elements for the kernels (one
    block takes one chunk), with the scratch the LAMB launches need, all allocated here, once: a
    step allocates nothing and can be captured into a hipGraph. The decay is read once, here: a
    later change of ``param_groups[0]["weight_decay"]`` does not reach the table.

    Segments must start at multiples of 4 elements and own the float4 that holds their last element
    (``FlatParams(align=16)`` gives both): the kernels then touch whole float4s, and the gaps, where
    p = g = 0, stay 0.
    """

    def __init__(self, flat: FlatParams, weight_decay: float, no_decay=None, adapt: bool = True):
        excluded = {id(p) for p in (no_decay or ())}
        unknown = excluded - {id(p) for p in flat.params}
        if unknown:
            raise ValueError(f"no_decay holds {len(unknown)} parameter(s) that the optimizer does not update")
        self.flat = flat
        self.segments = [(o, p.numel()) for p, o in zip(flat.params, flat.offsets)]
        ends = sorted(o for o, _ in self.segments)[1:] + [flat.numel]
        for (o, n), end in zip(sorted(self.segments), ends):
            if o % 4 or o + (n + 3) // 4 * 4 > end:
                raise ValueError("per-tensor optimizers need segments that start at multiples of 4 elements and "
                                 "do not share a float4 (FlatParams(align=16))")
        self.wd = [0.0 if id(p) in excluded else float(weight_decay) for p in flat.params]
        self.adapt = [0 if (id(p) in excluded or not adapt) else 1 for p in flat.params]
        self.last_trust = torch.ones(len(self.segments), dtype=torch.float32, device=flat.device)
        self.dev = None
        if flat.device.type == "cuda":
            self._build_device(int(require_native().optim_chunk_elems()))

    def _build_device(self, C: int) -> None:
        c4 = C // 4
        chunks, tseg = [], []
        for t, (o, n) in enumerate(self.segments):
            first, n4 = o // 4, (n + 3) // 4
            tseg.append((len(chunks), (n4 + c4 - 1) // c4))
            for s in range(0, n4, c4):
                chunks.append((t, first + s, min(c4, n4 - s), 0))
        if self.flat.numel // 4 >= 2 ** 31:
            raise ValueError("flat buffer too long for the 32-bit segment table")
        d, nt = self.flat.device, len(self.segments)
        i32 = dict(dtype=torch.int32, device=d)
        f32 = dict(dtype=torch.float32, device=d)
        self.dev = dict(
            chunks=torch.tensor(chunks, dtype=torch.int32).reshape(-1, 4).to(d),
            tseg=torch.tensor(tseg, dtype=torch.int32).reshape(-1, 2).to(d),
            wd=torch.tensor(self.wd, **f32), adapt=torch.tensor(self.adapt, **i32),
            part=torch.zeros(max(len(chunks), 1), 2, **f32), norms=torch.zeros(max(nt, 1), 2, **f32))
        self.last_trust = torch.ones(nt, **f32)


class FusedOptimizer(torch.optim.Optimizer):
    kind_name = "sgd"

    def __init__(self, params, defaults: Dict[str, Any], flat: Optional[FlatParams] = None):
        super().__init__(params, defaults)
        self._seg: Optional[SegmentTable] = None  # set by the per-tensor optimizers (_init_segments)
        self.kind = KIND[self.kind_name]
        self._flats: List[FlatParams] = []
        for gi, group in enumerate(self.param_groups):
            ps = group["params"]
            # reuse the caller's flat buffer (e.g. DDP's, laid out in reverse order) when it holds
            # exactly this group's parameters: the update runs over the whole buffer, order is irrelevant
            if flat is not None and len(self.param_groups) == 1 and \
                    sorted(id(p) for p in flat.params) == sorted(id(p) for p in ps if p.requires_grad):
                fp = flat
            else:
                fp = FlatParams(ps)
            self._flats.append(fp)
        self._s1: List[Optional[torch.Tensor]] = [None] * len(self._flats)
        self._s2: List[Optional[torch.Tensor]] = [None] * len(self._flats)
        self._steps: List[int] = [0] * len(self._flats)
        self._lr_dev: List[Optional[torch.Tensor]] = [None] * len(self._flats)
        self._lr_dev_val: List[Optional[float]] = [None] * len(self._flats)
        self.grad_scale = 1.0  # applied to incoming gradients (e.g. AMP unscale)
        for gi in range(len(self._flats)):
            self._alloc_state(gi)

    # ------------------------------------------------------------------
    @property
    def flats(self) -> List[FlatParams]:
        return self._flats

    @property
    def per_tensor(self) -> bool:
        """True when the step goes through the segment table (LAMB, AdamW with exclusions)."""
        return self._seg is not None

    def _init_segments(self, no_decay, adapt: bool) -> None:
        """Per-tensor behaviour lives inside the ONE flat buffer: extra param groups would each get a
        FlatParams of their own and re-point the parameters away from the DDP flat buffer."""
        if len(self._flats) != 1:
            raise ValueError(f"{type(self).__name__} with per-tensor behaviour takes a single param group "
                             "(pass no_decay=[...] instead of param groups)")
        if hasattr(self._flats[0], "export_state"):
            raise ValueError(f"{type(self).__name__} with per-tensor behaviour cannot run on a ZeRO-1 shard: "
                             "shards cut tensors, and a sharded norm needs a collective")
        self._seg = SegmentTable(self._flats[0], self.param_groups[0]["weight_decay"], no_decay, adapt)

    def last_trust(self) -> torch.Tensor:
        """Per-tensor trust ratios of the last step, in the order of ``flats[0].params`` (1 for tensors
        that are not adapted, and before the first step)."""
        if self._seg is None:
            raise RuntimeError(f"{type(self).__name__} keeps no per-tensor trust ratios")
        return self._seg.last_trust.detach().clone()

    def _needs(self, group) -> tuple:
        s2 = self.kind in (1, 2, 4, 5)
        s1 = s2 or self.kind == 3 or (self.kind == 0 and group.get("momentum", 0.0) != 0.0)
        return s1, s2

    def _alloc_state(self, gi: int) -> None:
        fp = self._flats[gi]
        s1, s2 = self._needs(self.param_groups[gi])
        if s1 and self._s1[gi] is None:
            self._s1[gi] = torch.zeros_like(fp.data)
        if s2 and self._s2[gi] is None:
            self._s2[gi] = torch.zeros_like(fp.data)

    def state_buffers(self, gi: int = 0):
        return self._s1[gi], self._s2[gi]

    def lr_tensor(self, gi: int = 0) -> torch.Tensor:
        """Device scalar holding the group's current lr (kept in sync with group['lr'])."""
        fp = self._flats[gi]
        lr = float(self.param_groups[gi]["lr"])
        if self._lr_dev[gi] is None:
            self._lr_dev[gi] = torch.full((1,), lr, dtype=torch.float32, device=fp.device)
            self._lr_dev_val[gi] = lr
        elif self._lr_dev_val[gi] != lr:
            self._lr_dev[gi].fill_(lr)  # a tiny kernel with lr as an argument: graph/stream safe
            self._lr_dev_val[gi] = lr
        return self._lr_dev[gi]

    def hyper(self, gi: int = 0) -> Dict[str, Any]:
        g = self.param_groups[gi]
        betas = g.get("betas", (0.9, 0.999))
        return dict(kind=self.kind, lr=float(g["lr"]), momentum=float(g.get("momentum", 0.0)),
                    dampening=float(g.get("dampening", 0.0)), weight_decay=float(g.get("weight_decay", 0.0)),
                    beta1=float(betas[0]), beta2=float(betas[1]), eps=float(g.get("eps", 1e-8)),
                    lr_decay=float(g.get("lr_decay", 0.0)), grad_scale=float(self.grad_scale),
                    nesterov=bool(g.get("nesterov", False)), maximize=bool(g.get("maximize", False)))

    # ------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = False) -> None:  # keep grads as flat views
        for fp in self._flats:
            fp.rebind_grads()
            fp.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, fp in enumerate(self._flats):
            fp.rebind_params()
            fp.rebind_grads()
            self._alloc_state(gi)
            self._steps[gi] += 1
            h = self.hyper(gi)
            if fp.device.type == "cuda":
                C = require_native()
                shadow = fp.shadow if fp.shadow is not None and fp._shadow_ver == fp.data._version else None
                if self._seg is not None:
                    self._seg_step(C, gi, h, shadow)
                else:
                    C.flat_optim(fp.data, fp.grad, self._s1[gi], self._s2[gi], h["kind"], h["lr"], h["momentum"],
                                 h["dampening"], h["weight_decay"], h["beta1"], h["beta2"], h["eps"],
                                 h["lr_decay"], h["grad_scale"], h["nesterov"], h["maximize"], None, None, None,
                                 float(self._steps[gi]), shadow, None)
                if shadow is not None:
                    fp.mark_shadow_fresh()  # the kernel rewrote the bf16 copy of every updated weight
            elif self._seg is not None:
                _cpu_update_seg(h, float(self._steps[gi]), fp.data, fp.grad, self._s1[gi], self._s2[gi], self._seg)
            else:
                _cpu_update(h, float(self._steps[gi]), fp.data, fp.grad, self._s1[gi], self._s2[gi])
            fp.generation += 1  # weights changed: derived copies (fp8 casts) are stale
        return loss

    def _seg_step(self, C, gi: int, h: Dict[str, Any], shadow: Optional[torch.Tensor]) -> None:
        """The per-tensor device step: LAMB's three launches, or AdamW's segmented single launch."""
        fp, seg = self._flats[gi], self._seg
        if seg.dev is None or seg.flat is not fp:
            raise RuntimeError("the flat buffer moved after the optimizer was built: the segment table is stale")
        d, t = seg.dev, float(self._steps[gi])
        if self.kind == KIND["lamb"]:
            C.lamb_step(fp.data, fp.grad, self._s1[gi], self._s2[gi], d["chunks"], d["tseg"], d["wd"], d["adapt"],
                        d["part"], d["norms"], seg.last_trust, h["lr"], h["beta1"], h["beta2"], h["eps"],
                        h["grad_scale"], h["maximize"], None, None, None, t, shadow, None, None, 0, 7)
        else:
            C.flat_optim_seg(fp.data, fp.grad, self._s1[gi], self._s2[gi], d["chunks"], d["wd"], h["lr"],
                             h["beta1"], h["beta2"], h["eps"], h["grad_scale"], h["maximize"], None, None, None, t,
                             shadow, None, None, 0)

    # ------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        groups = []
        for g in self.param_groups:
            groups.append({k: v for k, v in g.items() if k != "params"})
        return {"kind": self.kind_name, "param_groups": groups,
                "flat_state": [{"step": self._steps[i],
                                "s1": self._export(i, self._s1[i]), "s2": self._export(i, self._s2[i])}
                               for i in range(len(self._flats))]}

    def _export(self, i: int, buf: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if buf is None:
            return None
        fp = self._flats[i]
        # a ZeRO shard (parallel/zero.py) gathers its state into the full flat layout (collective)
        return fp.export_state(buf) if hasattr(fp, "export_state") else buf.detach().cpu()

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        if sd.get("kind") != self.kind_name:
            raise ValueError(f"optimizer kind mismatch: {sd.get('kind')} vs {self.kind_name}")
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k, v in sg.items():
                g[k] = v
        for i, st in enumerate(sd["flat_state"]):
            self._steps[i] = int(st["step"])
            for name, buf in (("s1", self._s1), ("s2", self._s2)):
                if st[name] is not None:
                    if buf[i] is None:
                        buf[i] = torch.zeros_like(self._flats[i].data)
                    if hasattr(self._flats[i], "import_state"):
                        self._flats[i].import_state(st[name], buf[i])
                    else:
                        buf[i].copy_(st[name].to(buf[i].device))
            self._lr_dev_val[i] = None if self._lr_dev[i] is None else -1.0


def _cpu_update(h, t, p, g, s1, s2) -> None:
    """Reference math for CPU flat buffers (mirrors mlt_optim.h)."""
    g = g * h["grad_scale"]
    if h["maximize"]:
        g = -g
    lr, wd, k = h["lr"], h["weight_decay"], h["kind"]
    if k == 0:
        if wd:
            g = g + wd * p
        if h["momentum"]:
            if t <= 1:
                s1.copy_(g)
            else:
                s1.mul_(h["momentum"]).add_(g, alpha=1 - h["dampening"])
            g = g + h["momentum"] * s1 if h["nesterov"] else s1
        p.add_(g, alpha=-lr)
    elif k in (1, 2):
        if k == 2:
            p.mul_(1 - lr * wd)
        elif wd:
            g = g + wd * p
        s1.lerp_(g, 1 - h["beta1"])
        s2.mul_(h["beta2"]).addcmul_(g, g, value=1 - h["beta2"])
        bc1 = 1 - h["beta1"] ** t
        bc2 = 1 - h["beta2"] ** t
        denom = (s2.sqrt() / math.sqrt(bc2)).add_(h["eps"])
        p.addcdiv_(s1, denom, value=-lr / bc1)
    elif k == 3:
        if wd:
            g = g + wd * p
        clr = lr / (1 + (t - 1) * h["lr_decay"])
        s1.addcmul_(g, g, value=1)
        p.addcdiv_(g, s1.sqrt().add_(h["eps"]), value=-clr)
    elif k == 4:
        if wd:
            g = g + wd * p
        s1.lerp_(g, 1 - h["beta1"])
        torch.maximum(s2.mul_(h["beta2"]), g.abs().add_(h["eps"]), out=s2)
        p.addcdiv_(s1, s2, value=-lr / (1 - h["beta1"] ** t))


def _cpu_update_seg(h, t, p, g, s1, s2, seg: SegmentTable) -> None:
    """The per-tensor optimizers on CPU flat buffers, tensor by tensor over the segments (the gaps
    between them are never touched). AdamW: _cpu_update with the tensor's decay. LAMB (mirrors
    mlt_optim.h): Adam's moments, u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd_i w,
    r_i = |w_i| / |u_i| when the tensor is adapted and both norms are > 0, else 1, w -= lr r_i u."""
    lamb = h["kind"] == KIND["lamb"]
    for i, (o, n) in enumerate(seg.segments):
        pi, gi, mi, vi = p[o:o + n], g[o:o + n], s1[o:o + n], s2[o:o + n]
        if not lamb:
            _cpu_update(dict(h, weight_decay=seg.wd[i]), t, pi, gi, mi, vi)
            continue
        gi = gi * h["grad_scale"]
        if h["maximize"]:
            gi = -gi
        mi.lerp_(gi, 1 - h["beta1"])
        vi.mul_(h["beta2"]).addcmul_(gi, gi, value=1 - h["beta2"])
        bc1 = 1 - h["beta1"] ** t
        bc2 = 1 - h["beta2"] ** t
        u = (mi / bc1).div_((vi.sqrt() / math.sqrt(bc2)).add_(h["eps"])).add_(pi, alpha=seg.wd[i])
        wn, un = float(pi.norm()), float(u.norm())
        r = wn / un if (seg.adapt[i] and wn > 0 and un > 0) else 1.0
        seg.last_trust[i] = r
        pi.add_(u, alpha=-h["lr"] * r)


class FusedSGD(FusedOptimizer):
    kind_name = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 maximize=False, flat=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize), flat)


class FusedAdam(FusedOptimizer):
    kind_name = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False,
                 flat=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize),
                         flat)


class FusedAdamW(FusedOptimizer):
    kind_name = "adamw"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, no_decay=None,
                 maximize=False, flat=None):
        """no_decay: an iterable of parameters that take no weight decay (the usual BERT recipe: biases
        and LayerNorm gains / shifts). With it the device step is the segmented launch
        (``flat_optim_seg``), which reads a decay per tensor; without it, the plain flat launch."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize),
                         flat)
        if no_decay is not None:
            self._init_segments(list(no_decay), adapt=False)


class FusedLAMB(FusedOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning"): Adam's moments and a
    layer-wise trust ratio |w_i| / |u_i| on every tensor of the one flat buffer. Bias correction is
    always on; a tensor in ``no_decay`` gets no decay and no trust ratio, i.e. a plain Adam step
    (apex FusedLAMB with use_nvlamb=False). Three launches on the device (``csrc/kernels/optim.hip``).
    A global-norm clip is the caller's (``clip_grad_norm_flat``), as for the other optimizers."""
    kind_name = "lamb"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, no_decay=None,
                 maximize=False, flat=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize),
                         flat)
        self._init_segments(list(no_decay or ()), adapt=True)


class FusedAdagrad(FusedOptimizer):
    kind_name = "adagrad"

    def __init__(self, params, lr=1e-2, lr_decay=0.0, weight_decay=0.0, eps=1e-10, maximize=False, flat=None):
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, weight_decay=weight_decay, eps=eps,
                                      maximize=maximize), flat)


class FusedAdamax(FusedOptimizer):
    kind_name = "adamax"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False,
                 flat=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize),
                         flat)


OPTIMIZERS = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW, "adagrad": FusedAdagrad,
              "adamax": FusedAdamax, "lamb": FusedLAMB}
PER_TENSOR_OPTIMIZERS = ("adamw", "lamb")  # the names that accept no_decay


def build_optimizer(name: str, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                    flat: Optional[FlatParams] = None, no_decay_1d: bool = False) -> Optional[FusedOptimizer]:
    """Factory with the reference's name->optimizer mapping (src/trainer.py:123-138):
    only SGD takes momentum; the others get lr + weight_decay with torch defaults. ``lamb`` is this
    project's addition. no_decay_1d (adamw, lamb): every parameter with ndim <= 1 (biases, LayerNorm
    weight and bias) is excluded from weight decay and, under LAMB, from the trust ratio."""
    name = (name or "").lower()
    if no_decay_1d and name in OPTIMIZERS and name not in PER_TENSOR_OPTIMIZERS:
        raise ValueError(f"no_decay_1d needs a per-tensor optimizer ({'|'.join(PER_TENSOR_OPTIMIZERS)}), "
                         f"not {name!r}")
    if name in PER_TENSOR_OPTIMIZERS and (no_decay_1d or name == "lamb"):
        params = list(params)
        nd = [p for p in params if p.requires_grad and p.ndim <= 1] if no_decay_1d else None
        return OPTIMIZERS[name](params, lr=lr, weight_decay=weight_decay, no_decay=nd, flat=flat)
    if name == "sgd":
        return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, flat=flat)
    if name in OPTIMIZERS:
        return OPTIMIZERS[name](params, lr=lr, weight_decay=weight_decay, flat=flat)
    return None


def clip_grad_norm_flat(flat: FlatParams, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ over a flat gradient buffer: one fused
    sum-of-squares kernel + one scale, no host sync (returns the device norm). The sum runs in a
    fixed order (per-block partials added in block order): norm and clipped gradients are bitwise
    reproducible from run to run."""
    g = flat.grad
    if g.is_cuda:
        C = require_native()
        sq = torch.empty(1, dtype=torch.float32, device=g.device)  # overwritten by sq_norm
        coef = torch.empty(1, dtype=torch.float32, device=g.device)
        total = torch.empty(1, dtype=torch.float32, device=g.device)
        C.sq_norm(g, sq)
        C.clip_coef(sq, float(max_norm), coef, total)
        g.mul_(coef)
        return total.view(())
    total = g.norm()
    g.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    return total
