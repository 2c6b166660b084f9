"""LAMB: layer-wise adaptive moments (You et al., "Large Batch Optimization for
Deep Learning: Training BERT in 76 minutes", 2020).

Per tensor, with ``t`` the step count after this step::

    m = m + (1 - beta1) (g - m)             v = beta2 v + (1 - beta2) g^2
    u = (m / (1 - beta1^t)) / (sqrt(v) / sqrt(1 - beta2^t) + eps) + wd * w
    trust = ||w|| / ||u||   (1 when adapt is off or either norm is 0), at most trust_clip
    w = w - lr * trust * u

With ``adapt=False`` this is AdamW with decoupled decay; the usual BERT recipe
sets it for the 1-D / bias / norm parameters' group.

``step()`` below is the portable per-tensor implementation; wrapped by
``DistributedOptimizer`` the whole model is updated over the parameter arena
instead (``ops.fused_lamb_``: on a GPU the step tick and three HIP launches,
with a device-side step count).  The state keys are torch.optim.Adam's
(``step``, ``exp_avg``, ``exp_avg_sq``).
"""
from __future__ import annotations

import math

import torch
from torch.optim.optimizer import Optimizer


class LAMB(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True,
                 trust_clip=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid betas: {}".format(betas))
        if not eps > 0.0:
            raise ValueError("Invalid epsilon value: {} (must be positive)".format(eps))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if trust_clip is not None and trust_clip < 0.0:
            raise ValueError("Invalid trust_clip value: {}".format(trust_clip))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adapt=adapt, trust_clip=trust_clip)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr = group["lr"]
            b1, b2 = group["betas"]
            eps = group["eps"]
            wd = group["weight_decay"]
            clip = group.get("trust_clip") or 0.0
            for p in group["params"]:
                if p.grad is None:
                    continue
                w = p.data
                g = p.grad.data
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(w)
                    st["exp_avg_sq"] = torch.zeros_like(w)
                st["step"] += 1
                t = float(st["step"])
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.lerp_(g, 1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                denom = (v.sqrt() / math.sqrt(1.0 - b2 ** t)).add_(eps)
                u = (m / (1.0 - b1 ** t)).div_(denom).add_(w, alpha=wd)
                trust = 1.0
                if group.get("adapt", True):
                    wn = float(torch.linalg.vector_norm(w.double()))
                    un = float(torch.linalg.vector_norm(u.double()))
                    if wn > 0 and un > 0:
                        trust = wn / un
                if clip > 0:
                    trust = min(trust, clip)
                w.add_(u, alpha=-lr * trust)
        return loss
