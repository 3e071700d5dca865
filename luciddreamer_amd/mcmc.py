"""MCMC densification for a GaussianModel on the MI355X (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte
Carlo", 2024): a fixed budget of Gaussians instead of the clone / split / prune heuristic of `densify.py`.

    strategy = MCMCStrategy(cap_max=1_000_000)
    ...
    loss.backward()
    strategy.add_regularizer_grads(model)          # + opacity_reg mean(opacity) + scale_reg mean(scale), as gradients
    model.optimizer.step(); model.optimizer.zero_grad(set_to_none=True)
    strategy.step(model, iteration, lr_xyz)        # relocate + grow on schedule, position noise every iteration

Four parts: the number of Gaussians never exceeds `cap_max`; Gaussians whose opacity fell to `min_opacity` are relocated onto
live ones sampled by opacity; the set grows by `grow_rate` per refinement up to the cap; a position noise scaled by each
Gaussian's covariance is added after every optimizer step.  The view-space gradient is never thresholded and the densification
statistics are never read.  The arithmetic is in csrc/mcmc.hip (lr_mcmc_relocate, lr_mcmc_noise, lr_mcmc_reg_grad; formulas in
include/lucid_raster.h and DESIGN.md section 4b-MCMC); this module chooses the rows and keeps parameters and Adam moments views of
the model's row store (`densify.RowStore`), exactly as `densify.py` does.  `model` is the same duck-typed object; FusedAdam and
torch.optim.Adam both work.  Requires the HIP library (no CPU path).

`sampled_idx` (the source rows) and `noise` can be passed in, so that a data-parallel caller can give every rank the draws of
rank 0.
"""
import ctypes

import torch

from . import _lib
from . import densify

GROUPS = tuple(densify.GROUP_ATTR)          # xyz, f_dc, f_rest, opacity, scaling, rotation: the order of the C argument struct


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_device(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"luciddreamer_amd.mcmc: {what} must be on a HIP device (no CPU path)")


def _f32(t, what, numel=None):
    _need_device(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise RuntimeError(f"luciddreamer_amd.mcmc: {what} must be a contiguous float32 tensor" +
                           (f" of {numel} elements" if numel is not None else ""))
    return t


def _one_device(dev, *tensors):
    """Every pointer of a call is dereferenced on ONE device: the first tensor's."""
    for t in tensors:
        if t is not None and t.device != dev:
            raise RuntimeError(f"luciddreamer_amd.mcmc: all tensors of a call must be on one device ({dev}), got {t.device}")


def relocate_rows(dst, src, params, exp_avg=None, exp_avg_sq=None, *, rows=None, min_opacity=0.005, n_max=51, workspace=None):
    """lr_mcmc_relocate on tensors.  dst, src: int32 device tensors of n rows each ({dst} and {src} disjoint, dst without
    duplicates, every index below `rows` -- the caller's word, see the header); params / exp_avg / exp_avg_sq: {group: tensor}
    over GROUPS (moments optional, whole or per group); rows: how many rows the tensors can address (default: params["xyz"]'s).
    Returns the workspace it used, for reuse."""
    n = int(dst.numel())
    if int(src.numel()) != n:
        raise RuntimeError("luciddreamer_amd.mcmc: dst and src must have the same length")
    for t, what in ((dst, "dst"), (src, "src")):
        _need_device(t, what)
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError(f"luciddreamer_amd.mcmc: {what} must be a contiguous int32 tensor")
    dev = params["xyz"].device
    rows = int(params["xyz"].shape[0]) if rows is None else int(rows)
    n_rest = int(params["f_rest"].shape[1])
    width = {"xyz": 3, "f_dc": 3, "f_rest": 3 * n_rest, "opacity": 1, "scaling": 3, "rotation": 4}
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    for g in GROUPS:
        for d, what in ((params, g), (exp_avg, g + ".exp_avg"), (exp_avg_sq, g + ".exp_avg_sq")):
            if d is not None and d.get(g) is not None:
                if int(d[g].shape[0]) < rows:
                    raise RuntimeError(f"luciddreamer_amd.mcmc: {what} has fewer than {rows} rows")
                _one_device(dev, _f32(d[g], what, int(d[g].shape[0]) * width[g]))
    _one_device(dev, dst, src)
    L = _lib.lib()
    need = L.lr_mcmc_workspace_bytes(rows, n)
    if workspace is None or workspace.numel() < need or workspace.device != dev:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    moments = lambda d: (ctypes.c_void_p * 6)(*[ptr(d.get(g)) if d else None for g in GROUPS])
    a = _lib.McmcRelocateArgs(n=n, dst=ptr(dst), src=ptr(src), P_rows=rows, M=1 + n_rest,
                              xyz=ptr(params["xyz"]), features_dc=ptr(params["f_dc"]), features_rest=ptr(params["f_rest"]),
                              opacity=ptr(params["opacity"]), scaling=ptr(params["scaling"]), rotation=ptr(params["rotation"]),
                              exp_avg=moments(exp_avg), exp_avg_sq=moments(exp_avg_sq),
                              min_opacity=float(min_opacity), n_max=int(n_max),
                              workspace=workspace.data_ptr(), workspace_bytes=workspace.numel(), stream=_stream(dev))
    with _lib.on_device(dev):
        rc = L.lr_mcmc_relocate(a)
    if rc < 0:
        _lib.raise_for(rc, "lr_mcmc_relocate")
    return workspace


def add_noise(xyz, raw_scale, raw_rotation, raw_opacity, noise, scaler):
    """lr_mcmc_noise: xyz += Sigma noise g(opacity) scaler, in place."""
    P = int(xyz.shape[0])
    _f32(xyz, "xyz", 3 * P), _f32(raw_scale, "scaling", 3 * P), _f32(raw_rotation, "rotation", 4 * P)
    _f32(raw_opacity, "opacity", P), _f32(noise, "noise", 3 * P)
    dev = xyz.device
    _one_device(dev, raw_scale, raw_rotation, raw_opacity, noise)
    with _lib.on_device(dev):
        rc = _lib.lib().lr_mcmc_noise(P, xyz.data_ptr(), raw_scale.data_ptr(), raw_rotation.data_ptr(), raw_opacity.data_ptr(),
                                      noise.data_ptr(), float(scaler), _stream(dev))
    if rc < 0:
        _lib.raise_for(rc, "lr_mcmc_noise")


def add_reg_grad(raw_opacity, raw_scale, opacity_reg, scale_reg, dL_dopacity, dL_dscale):
    """lr_mcmc_reg_grad: the gradient of opacity_reg mean(sigmoid(opacity)) + scale_reg mean(exp(scaling)) ADDED to the two
    gradient tensors."""
    P = int(raw_opacity.shape[0])
    _f32(raw_opacity, "opacity", P), _f32(raw_scale, "scaling", 3 * P)
    _f32(dL_dopacity, "the opacity gradient", P), _f32(dL_dscale, "the scaling gradient", 3 * P)
    dev = raw_opacity.device
    _one_device(dev, raw_scale, dL_dopacity, dL_dscale)
    with _lib.on_device(dev):
        rc = _lib.lib().lr_mcmc_reg_grad(P, raw_opacity.data_ptr(), raw_scale.data_ptr(), float(opacity_reg), float(scale_reg),
                                         dL_dopacity.data_ptr(), dL_dscale.data_ptr(), _stream(dev))
    if rc < 0:
        _lib.raise_for(rc, "lr_mcmc_reg_grad")


class MCMCStrategy:
    def __init__(self, cap_max, noise_lr=5e5, min_opacity=0.005, grow_rate=1.05, n_max=51, opacity_reg=0.01, scale_reg=0.01,
                 refine_start=500, refine_stop=25_000, refine_every=100):
        if int(cap_max) < 1 or not (1 <= int(n_max) <= 51) or grow_rate < 1.0 or not (0.0 < min_opacity < 1.0):
            raise ValueError("MCMCStrategy: cap_max >= 1, n_max in [1, 51], grow_rate >= 1 and 0 < min_opacity < 1 required")
        self.cap_max, self.noise_lr, self.min_opacity = int(cap_max), float(noise_lr), float(min_opacity)
        self.grow_rate, self.n_max = float(grow_rate), int(n_max)
        self.opacity_reg, self.scale_reg = float(opacity_reg), float(scale_reg)
        self.refine_start, self.refine_stop, self.refine_every = int(refine_start), int(refine_stop), int(refine_every)
        self._ws = None

    # ---- arithmetic that needs no device --------------------------------------------------------------------------------
    def n_new(self, P):
        """Rows a growth round adds to P: grow_rate per round, never beyond cap_max."""
        return max(0, min(self.cap_max, int(self.grow_rate * P)) - int(P))

    # ---- helpers --------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_model(model):
        for a in densify.GROUP_ATTR.values():
            _need_device(getattr(model, a), a)

    def _sources(self, probs, count, generator, sampled_idx, rows, candidates=None):
        """`count` source rows: given, or drawn with replacement with probability proportional to `probs` (over `candidates`)."""
        if sampled_idx is not None:
            _need_device(sampled_idx, "sampled_idx")
            s = sampled_idx.reshape(-1).to(torch.int64)
            if s.numel() != count:
                raise RuntimeError(f"luciddreamer_amd.mcmc: sampled_idx has {s.numel()} entries, this round needs {count}")
            if count and (int(s.min()) < 0 or int(s.max()) >= rows):
                raise RuntimeError("luciddreamer_amd.mcmc: sampled_idx out of range")
            return s
        pick = torch.multinomial(probs, count, replacement=True, generator=generator)
        return pick if candidates is None else candidates[pick]

    def _apply(self, model, st, dst, src, rows):
        """One lr_mcmc_relocate over the store's buffers (parameters and whatever moments the optimizer has created)."""
        moments = lambda key: {g: st.bufs.get(f"{g}.{key}") for g in GROUPS}
        self._ws = relocate_rows(dst.to(torch.int32).contiguous(), src.to(torch.int32).contiguous(),
                                 {g: st.bufs[g] for g in GROUPS}, moments("exp_avg"), moments("exp_avg_sq"), rows=rows,
                                 min_opacity=self.min_opacity, n_max=self.n_max, workspace=self._ws)

    # ---- the four parts -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def relocate(self, model, generator=None, sampled_idx=None):
        """Move every dead Gaussian (sigmoid(opacity) <= min_opacity) onto a live one drawn with probability proportional to
        its opacity; the source and its copies share the source's opacity and scale by the paper's rule.  Returns the number
        moved (0 when no row is dead or none is alive).  Gradients of the parameters are dropped, as by every row surgery."""
        self._check_model(model)
        densify._no_fused_step_pending(model)
        opacity = torch.sigmoid(model._opacity.detach()).reshape(-1)
        dead = opacity <= self.min_opacity
        dst = dead.nonzero().reshape(-1)
        P, n = int(opacity.numel()), int(dst.numel())
        if n == 0 or n == P:
            return 0
        alive = (~dead).nonzero().reshape(-1)
        src = self._sources(opacity[alive], n, generator, sampled_idx, P, alive)
        if sampled_idx is not None and bool(dead[src].any()):
            raise RuntimeError("luciddreamer_amd.mcmc: sampled_idx names a dead row as a source")
        st = densify._store(model)
        self._apply(model, st, dst, src, st.P)
        densify._bind(model, st)
        return n

    @torch.no_grad()
    def grow(self, model, generator=None, sampled_idx=None):
        """Append n_new(P) Gaussians, each a copy of a row drawn with probability proportional to its opacity, with opacity and
        scale shared as in relocate.  The statistics rows of the new Gaussians are zero.  Returns the number added."""
        self._check_model(model)
        densify._no_fused_step_pending(model)
        P = int(model._xyz.shape[0])
        n = self.n_new(P)
        if n == 0:
            return 0
        opacity = torch.sigmoid(model._opacity.detach()).reshape(-1)
        src = self._sources(opacity, n, generator, sampled_idx, P)
        st = densify._store(model)
        st.ensure_capacity(P + n)
        dst = torch.arange(P, P + n, dtype=torch.int32, device=src.device)
        self._apply(model, st, dst, src, P + n)
        for a in densify.STAT_ATTRS:
            st.bufs[a][P:P + n].zero_()
        st.P = P + n
        densify._bind(model, st)
        return n

    @torch.no_grad()
    def add_regularizer_grads(self, model):
        """Add the gradients of the two regularisers to model._opacity.grad and model._scaling.grad (after backward, before the
        optimizer's step); a missing gradient starts from zero."""
        self._check_model(model)
        for p in (model._opacity, model._scaling):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        add_reg_grad(model._opacity.detach(), model._scaling.detach(), self.opacity_reg, self.scale_reg,
                     _f32(model._opacity.grad, "opacity.grad"), _f32(model._scaling.grad, "scaling.grad"))

    @torch.no_grad()
    def inject_noise(self, model, lr_xyz, noise=None, generator=None):
        """xyz += Sigma noise g(opacity) noise_lr lr_xyz: after the optimizer's step, every iteration."""
        self._check_model(model)
        xyz = model._xyz.detach()
        if noise is None:
            noise = torch.randn(xyz.shape, dtype=torch.float32, device=xyz.device, generator=generator)
        add_noise(xyz, model._scaling.detach(), model._rotation.detach(), model._opacity.detach(), noise, self.noise_lr * float(lr_xyz))

    def step(self, model, iteration, lr_xyz, refine_start=None, refine_stop=None, refine_every=None, generator=None):
        """After the optimizer's step of `iteration`: relocate and grow when refine_start <= iteration < refine_stop and
        iteration is a multiple of refine_every (default: the constructor's schedule, 500 / 25000 / 100), then the position
        noise.  Returns (relocated, added)."""
        refine_start = self.refine_start if refine_start is None else refine_start
        refine_stop = self.refine_stop if refine_stop is None else refine_stop
        refine_every = self.refine_every if refine_every is None else refine_every
        moved = added = 0
        if refine_start <= iteration < refine_stop and iteration % refine_every == 0:
            moved = self.relocate(model, generator=generator)
            added = self.grow(model, generator=generator)
        self.inject_noise(model, lr_xyz, generator=generator)
        return moved, added
