"""Optimizer side of the training step on gfx950 kernels: AdamW with the
constructor of ``torch.optim.AdamW`` (seaweed_apt/distilled_trainer.py:69-75),
the EMA update of distilled_trainer.py:319-334 kept on the GPU, and the global
gradient-norm clip of Omnihuman/omnihuman_trainer.py:349-356, on its own
(``clip_grad_norm_``) or inside the optimizer step (``AdamW(max_grad_norm=)``)."""
import os
import weakref

import torch

from . import ops

# OMH_ADAMW_PACK=0: the bf16 operand copies of the training step in their own launch after the step (round 3), not
# written by the optimizer kernel (A/B timing)
try:
    from .wan.modules.model_train import pack_entry_of
except Exception:  # pragma: no cover
    pack_entry_of = None


def _norm_plan(cache, key, rows, dev):
    """The device table {grad, numel, first chunk} of omh_grad_norm_multi / omh_scale_multi for ``rows`` = [(grad address,
    numel)] and the workspace of one fp32 partial per chunk: (rows, table, total chunks, workspace), rebuilt and
    re-uploaded only when an address or a size changed."""
    ent = cache.get(key)
    if ent is None or ent[0] != rows:
        full, chunk0 = [], 0
        for g_, n_ in rows:
            full.append([g_, n_, chunk0])
            chunk0 += (n_ + ops.NORM_CHUNK - 1) // ops.NORM_CHUNK
        ws = ent[3] if ent is not None and ent[3].numel() >= chunk0 else torch.empty(chunk0, dtype=torch.float32, device=dev)
        ent = cache[key] = (rows, torch.tensor(full, dtype=torch.int64).to(dev, non_blocking=False), chunk0, ws)
    return ent


_CLIP_TABLES = {}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` (omnihuman_trainer.py:349-353) in two launches for all gradients together:
    omh_grad_norm_multi leaves the global L2 norm and min(1, max_norm / (norm + 1e-6)) on the device, omh_scale_multi
    multiplies every gradient by that coefficient in place (and touches nothing when it is 1).  Returns the norm before
    clipping as a 0-d fp32 tensor on the gradients' device; nothing is read back to the host unless
    ``error_if_nonfinite`` asks for the check.  Gradients must be fp32, contiguous and on one device; only the L2 norm is
    built; ``foreach`` is accepted for torch's signature and ignored."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: only the L2 norm is implemented on the device, got norm_type={norm_type!r}")
    max_norm = float(max_norm)
    rows, grads = [], []
    for i, p in enumerate(parameters):
        g = p.grad
        if g is None:
            continue
        what = f"the gradient of parameter {i} (shape {tuple(g.shape)}, {g.dtype}, {g.device})"
        ops._dev(g)
        if g.dtype != torch.float32:
            raise ValueError(f"clip_grad_norm_: {what} must be float32")
        if not g.is_contiguous():
            raise ValueError(f"clip_grad_norm_: {what} must be contiguous (strides {tuple(g.stride())})")
        if grads and g.device != grads[0].device:
            raise ValueError(f"clip_grad_norm_: {what} is not on {grads[0].device} with the gradients before it")
        if g.numel():
            grads.append(g)
            rows.append((g.data_ptr(), g.numel()))
    if not rows:
        return torch.tensor(0.0)
    dev = grads[0].device
    _, table, chunks, ws = _norm_plan(_CLIP_TABLES, (dev, len(rows)), rows, dev)
    if len(_CLIP_TABLES) > 8:
        _CLIP_TABLES.pop(next(iter(_CLIP_TABLES)))
    out = torch.empty(2, dtype=torch.float32, device=dev)       # a fresh pair per call: the caller keeps the norm
    with torch.cuda.device(dev):
        ops.grad_norm_multi(table, len(rows), chunks, ws, out, max_norm)
        if error_if_nonfinite and not bool(torch.isfinite(out[0])):
            raise RuntimeError(
                f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be "
                "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                "`error_if_nonfinite=False`")
        ops.scale_multi(table, len(rows), chunks, out[1:])
    torch.autograd.graph.increment_version(grads)
    return out[0]


# ------------------------------------------------------------------------------------- FP8 block-scaled moments
# include/omh.h states the format: uint8 e4m3fn codes [rows, cols] + fp32 scales [rows, ceil(cols / 64)] per moment, the
# second moment kept as its root.
_STATE8 = ("exp_avg_q", "exp_avg_scale", "exp_avg_sq_root_q", "exp_avg_sq_root_scale")


def _view8(p):
    """[rows, cols] of a parameter with 8-bit moments: the pack tables' view of Linear and patch-embedding weights."""
    rows = p.shape[0]
    return rows, p.numel() // rows


def _tiles8(rows, cols):
    return ((rows + 63) // 64) * ((cols + 63) // 64)


def _convert_moments(fp32s, codes, scales, second_moment, quantize):
    """One omh_moments_quantize / omh_moments_dequantize launch over the triples (fp32 [rows, cols], codes, scales)."""
    if not fp32s:
        return
    full, tile0 = [], 0
    for x, q, sc in zip(fp32s, codes, scales):
        rows, cols = q.shape
        assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == rows * cols
        assert q.dtype == torch.uint8 and q.is_contiguous() and sc.dtype == torch.float32 and sc.is_contiguous()
        assert tuple(sc.shape) == (rows, (cols + 63) // 64) and x.device == q.device == sc.device
        full.append([x.data_ptr(), q.data_ptr(), sc.data_ptr(), rows, cols, tile0])
        tile0 += _tiles8(rows, cols)
    dev = fp32s[0].device
    with torch.cuda.device(dev):
        table = torch.tensor(full, dtype=torch.int64).to(dev)
        (ops.moments_quantize if quantize else ops.moments_dequantize)(table, len(full), tile0, second_moment)


def quantize_moments(tensors, second_moment):
    """fp32 moments (each viewed as [shape[0], numel // shape[0]]) -> [(codes uint8 [rows, cols], scales fp32 [rows,
    ceil(cols / 64)])] on their device, one launch per device; ``second_moment``: the tensors hold v, the codes sqrt(v)."""
    out, by_dev = [], {}
    for t in tensors:
        rows, cols = _view8(t)
        x = t.detach().to(torch.float32).contiguous()
        q = torch.empty(rows, cols, dtype=torch.uint8, device=t.device)
        sc = torch.empty(rows, (cols + 63) // 64, dtype=torch.float32, device=t.device)
        out.append((q, sc))
        by_dev.setdefault(t.device, []).append((x, q, sc))
    for trip in by_dev.values():
        _convert_moments(*zip(*trip), second_moment, True)
    return out


def dequantize_moments(pairs, second_moment, shapes=None):
    """[(codes, scales)] -> fp32 moments (``second_moment``: v, the square of what the codes decode to), each reshaped to
    ``shapes[i]`` where given."""
    out, by_dev = [], {}
    for i, (q, sc) in enumerate(pairs):
        q = q.contiguous()
        sc = sc.to(torch.float32).contiguous()
        x = torch.empty(q.shape, dtype=torch.float32, device=q.device)
        out.append(x if shapes is None else x.view(shapes[i]))
        by_dev.setdefault(q.device, []).append((x, q, sc))
    for trip in by_dev.values():
        _convert_moments(*zip(*trip), second_moment, False)
    return out


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW``-compatible (lr, betas, eps, weight_decay); one fused kernel per parameter.

    ``max_grad_norm`` (omnihuman_trainer.py:349-356, omni_config.yaml:44): ``step()`` clips the global L2 norm of the
    gradients of all parameter groups to it, as ``clip_grad_norm_(model.parameters(), max_grad_norm)`` before the step
    would — one omh_grad_norm_multi launch, then the AdamW kernels multiply the gradients they read by the coefficient
    that launch left on the device.  ``p.grad`` itself is NOT scaled: that is the one visible difference from
    clip-then-step.  ``grad_norm`` holds the norm before clipping of the last such step as a 0-d device tensor (for
    logging without a synchronisation).  ``max_grad_norm`` is an attribute of the optimizer, not a hyper-parameter of
    the groups: ``state_dict()`` is what it is without it, and a ``torch.optim.AdamW`` state dict loads.

    ``moments="fp8"``: a parameter with ``dim() >= 2`` and ``numel() >= min_8bit_size`` keeps its two moments as FP8
    block-scaled codes (include/omh.h: 2.125 bytes per weight instead of 8; state keys ``exp_avg_q``, ``exp_avg_scale``,
    ``exp_avg_sq_root_q``, ``exp_avg_sq_root_scale``) and is stepped by omh_adamw8_pack_multi; every other parameter, and
    one whose first gradient is not contiguous, keeps fp32 moments and the launches of ``moments="fp32"``, bit for bit.
    Both are attributes of the optimizer like ``max_grad_norm``.  ``state_dict(dequantize=True)`` returns fp32
    ``exp_avg`` / ``exp_avg_sq`` that ``torch.optim.AdamW`` loads; ``load_state_dict`` takes either form into either mode."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 moments="fp32", min_8bit_size=4096):
        if moments not in ("fp32", "fp8"):
            raise ValueError(f"AdamW: moments must be 'fp32' or 'fp8', got {moments!r}")
        if isinstance(min_8bit_size, bool) or not isinstance(min_8bit_size, int) or min_8bit_size < 0:
            raise ValueError(f"AdamW: min_8bit_size must be a non-negative integer, got {min_8bit_size!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self.moments = moments
        self.min_8bit_size = min_8bit_size
        # model_train.pending_step_bytes reads the bytes per element the moments of a parameter WILL take (default 8)
        for group in self.param_groups:
            for p in group["params"]:
                if moments == "fp8" and self._eligible8(p):
                    rows, cols = _view8(p)
                    p._omh_moment_bytes = (2 * p.numel() + 8 * rows * ((cols + 63) // 64)) / p.numel()
                else:
                    p.__dict__.pop("_omh_moment_bytes", None)

    def _eligible8(self, p):
        return (self.moments == "fp8" and p.dim() >= 2 and p.numel() >= max(1, self.min_8bit_size)
                and p.dtype == torch.float32 and p.is_contiguous())

    @staticmethod
    def _zeros8(p):
        rows, cols = _view8(p)
        nb = (cols + 63) // 64
        return {"exp_avg_q": torch.zeros(rows, cols, dtype=torch.uint8, device=p.device),
                "exp_avg_scale": torch.zeros(rows, nb, dtype=torch.float32, device=p.device),
                "exp_avg_sq_root_q": torch.zeros(rows, cols, dtype=torch.uint8, device=p.device),
                "exp_avg_sq_root_scale": torch.zeros(rows, nb, dtype=torch.float32, device=p.device)}

    def _params_by_index(self):
        """state_dict()'s parameter numbering: position in the concatenation of the groups."""
        return dict(enumerate(p for group in self.param_groups for p in group["params"]))

    def state_dict(self, dequantize=False):
        """``dequantize=True``: what ``torch.optim.AdamW`` keeps and loads — 8-bit moments as fp32 ``exp_avg`` /
        ``exp_avg_sq`` (converted on the device) and ``step`` as a 0-d fp32 tensor."""
        sd = super().state_dict()
        if not dequantize:
            return sd
        for i, st in sd["state"].items():
            sd["state"][i] = dict(st, step=torch.tensor(float(st["step"]), dtype=torch.float32))
        params = self._params_by_index()
        idx = [i for i, st in sd["state"].items() if "exp_avg_q" in st]
        if idx:
            shapes = [params[i].shape for i in idx]
            m = dequantize_moments([(sd["state"][i]["exp_avg_q"], sd["state"][i]["exp_avg_scale"]) for i in idx], False, shapes)
            v = dequantize_moments([(sd["state"][i]["exp_avg_sq_root_q"], sd["state"][i]["exp_avg_sq_root_scale"])
                                    for i in idx], True, shapes)
            for i, m_, v_ in zip(idx, m, v):
                st = {k: x for k, x in sd["state"][i].items() if k not in _STATE8}
                st["exp_avg"], st["exp_avg_sq"] = m_, v_
                sd["state"][i] = st
        return sd

    def load_state_dict(self, state_dict):
        """Either layout into either mode.  torch casts every state tensor but ``step`` to the parameter's dtype, so the
        codes arrive as fp32 holding 0 ... 255 (exactly): they are made uint8 again, then the state of every parameter
        is converted to what this optimizer's mode keeps for it."""
        super().load_state_dict(state_dict)
        to8, to32 = [], []
        for p, st in self.state.items():
            if "exp_avg_q" in st:
                for k in ("exp_avg_q", "exp_avg_sq_root_q"):
                    st[k] = st[k].to(torch.uint8).contiguous()
                for k in ("exp_avg_scale", "exp_avg_sq_root_scale"):
                    st[k] = st[k].to(torch.float32).contiguous()
                if not self._eligible8(p):
                    to32.append((p, st))
            elif "exp_avg" in st and self._eligible8(p) and st["exp_avg"].is_cuda:
                to8.append((p, st))
        if to8:
            m = quantize_moments([st["exp_avg"] for _, st in to8], False)
            v = quantize_moments([st["exp_avg_sq"] for _, st in to8], True)
            for (p, st), (mq, ms), (rq, rs) in zip(to8, m, v):
                del st["exp_avg"], st["exp_avg_sq"]
                st["exp_avg_q"], st["exp_avg_scale"], st["exp_avg_sq_root_q"], st["exp_avg_sq_root_scale"] = mq, ms, rq, rs
        if to32:
            shapes = [p.shape for p, _ in to32]
            m = dequantize_moments([(st["exp_avg_q"], st["exp_avg_scale"]) for _, st in to32], False, shapes)
            v = dequantize_moments([(st["exp_avg_sq_root_q"], st["exp_avg_sq_root_scale"]) for _, st in to32], True, shapes)
            for (p, st), m_, v_ in zip(to32, m, v):
                for k in _STATE8:
                    del st[k]
                st["exp_avg"], st["exp_avg_sq"] = m_, v_
        for p, st in self.state.items():
            mo = st.get("exp_avg_q", st.get("exp_avg"))
            if mo is not None:
                p._omh_moments_allocated = weakref.ref(mo)

    def _global_norm(self, grad_scale):
        """One norm launch over the gradients of every group; returns ({id(p): the gradient the step reads}, coef)."""
        grads, rows = {}, []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None or id(p) in grads:
                    continue
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                assert g.dtype == torch.float32, "max_grad_norm: gradients must be float32"
                if rows and g.device != dev:
                    raise ValueError(f"AdamW(max_grad_norm=): gradients on {dev} and {g.device}; the global norm is "
                                     "built on one device")
                dev = g.device
                grads[id(p)] = g
                if g.numel():
                    rows.append((g.data_ptr(), g.numel()))
        if not rows:
            return grads, None
        _, table, chunks, ws = _norm_plan(self.__dict__.setdefault("_tables", {}), (dev, len(rows), "norm"), rows, dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)   # fresh per step: grad_norm stays valid for the caller
        with torch.cuda.device(dev):
            ops.grad_norm_multi(table, len(rows), chunks, ws, out, self.max_grad_norm, grad_scale)
        self.grad_norm = out[0]
        return grads, out[1:]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        clipped, coef = None, None
        if getattr(self, "max_grad_norm", None) is not None:
            clipped, coef = self._global_norm(grad_scale)
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            by_step = {}
            by_step8 = {}                                   # rows with FP8 block-scaled moments: their own launch
            keep = []                                       # keeps .contiguous() copies alive until the launch
            touched = []
            marks = []                                      # (TrainPacks, row): copies this step writes itself
            fuse = os.environ.get("OMH_ADAMW_PACK", "1") != "0" and pack_entry_of is not None
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st and self._eligible8(p) and p.grad.dtype == torch.float32 and p.grad.is_contiguous():
                    st["step"] = 0
                    st.update(self._zeros8(p))
                    p._omh_moments_allocated = weakref.ref(st["exp_avg_q"])
                elif not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    # model_train.pending_step_bytes stops counting them while they are alive (weak: a deleted optimizer
                    # frees them again)
                    p._omh_moments_allocated = weakref.ref(st["exp_avg"])
                # a state dict saved by torch.optim.AdamW (the 'optimizer' entry of the reference's checkpoints,
                # distilled_trainer.py:153-178) holds the step as a 0-d tensor: normalise to a Python int
                st["step"] = int(st["step"]) + 1
                if clipped is not None:
                    g = clipped[id(p)]                          # the very tensor the norm was taken of
                else:
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                touched.append(p)
                assert p.dtype == torch.float32 and p.is_contiguous() and g.dtype == torch.float32
                if "exp_avg_q" in st:
                    rows8, cols8 = _view8(p)
                    row = (p.data_ptr(), g.data_ptr()) + tuple(st[k].data_ptr() for k in _STATE8)
                    ent = pack_entry_of(p) if fuse else None
                    pr = ent[0].rows[ent[1]] if ent is not None else None
                    if pr is not None and pr[8] == 0 and (pr[3], pr[4]) == (rows8, cols8):
                        row += (pr[1], pr[2], rows8, cols8, pr[5], pr[6])
                        marks.append(ent)
                    else:                                       # a plain weight: no copies (or none this pass can write)
                        row += (0, 0, rows8, cols8, 0, 0)
                    by_step8.setdefault((st["step"], p.device), []).append(row)
                    continue
                row = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                ent = pack_entry_of(p) if fuse else None
                if ent is not None:                             # this weight has bf16 operand copies for the training step
                    packs, ri = ent
                    pr = packs.rows[ri]                          # [src, dst, dstT, rows, cols, ld_dst, ld_t, tile0, kind]
                    row = row + (pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], 0 if pr[8] == 0 else 1)
                    marks.append((packs, ri))
                by_step.setdefault((st["step"], p.device), []).append(row)
            for (step, dev), rows in by_step8.items():
                cache = self.__dict__.setdefault("_tables", {})
                key = (gi, dev, len(rows), "fp8")
                ent = cache.get(key)
                if ent is None or ent[0] != rows:               # as below: uploaded again only when an address changed
                    full, tile0 = [], 0
                    for r in rows:
                        full.append(list(r) + [tile0])
                        tile0 += _tiles8(r[8], r[9])
                    ent = cache[key] = (rows, torch.tensor(full, dtype=torch.int64).to(dev, non_blocking=False), tile0)
                with torch.cuda.device(dev):
                    if coef is not None:
                        ops.adamw8_pack_multi_dev(ent[1], len(rows), ent[2], group["lr"], b1, b2, group["eps"],
                                                  group["weight_decay"], step, coef, grad_scale)
                    else:
                        ops.adamw8_pack_multi(ent[1], len(rows), ent[2], group["lr"], b1, b2, group["eps"],
                                              group["weight_decay"], step, grad_scale)
            # one multi-tensor launch per (step count, device): ~750 parameter tensors -> 1 kernel
            for (step, dev), rows in by_step.items():
                # the pointer table is re-uploaded only when an address changed (never under a graphed step,
                # whose gradients live at fixed addresses): no host-to-device copy in the steady state
                cache = self.__dict__.setdefault("_tables", {})
                # keyed per parameter group and device; parameters that joined later (a different step count) get
                # their own table instead of evicting the main one every step
                if any(len(r) > 5 for r in rows):
                    # AdamW + the bf16 operand copies in one pass (omh_adamw_pack_multi): 12-column table with the first
                    # tile of every entry (64 x 64 tiles for weights with copies, 4096-element chunks otherwise)
                    key = (gi, dev, len(rows), "pack")
                    ent = cache.get(key)
                    if ent is None or ent[0] != rows:
                        full, tile0 = [], 0
                        for r in rows:
                            if len(r) > 5 and r[11] == 0:
                                e_ = [r[0], r[1], r[2], r[3], r[5], r[6], r[7], r[8], r[9], r[10], tile0, 0]
                                tile0 += ((r[7] + 63) // 64) * ((r[8] + 63) // 64)
                            elif len(r) > 5:
                                e_ = [r[0], r[1], r[2], r[3], r[5], 0, 1, r[4], 0, 0, tile0, 1]
                                tile0 += (r[4] + 4095) // 4096
                            else:
                                e_ = [r[0], r[1], r[2], r[3], 0, 0, 1, r[4], 0, 0, tile0, 2]
                                tile0 += (r[4] + 4095) // 4096
                            full.append(e_)
                        ent = cache[key] = (rows, torch.tensor(full, dtype=torch.int64).to(dev, non_blocking=False), tile0)
                    if coef is not None:
                        ops.adamw_pack_multi_dev(ent[1], len(rows), ent[2], group["lr"], b1, b2, group["eps"],
                                                 group["weight_decay"], step, coef, grad_scale)
                    else:
                        ops.adamw_pack_multi(ent[1], len(rows), ent[2], group["lr"], b1, b2, group["eps"],
                                             group["weight_decay"], step, grad_scale)
                    continue
                key = (gi, dev, len(rows))
                ent = cache.get(key)
                if ent is None or ent[0] != rows:
                    ent = cache[key] = (rows, torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=False))
                table = ent[1]
                if coef is not None:
                    ops.adamw_multi_dev(table, len(rows), group["lr"], b1, b2, group["eps"], group["weight_decay"], step,
                                        coef, grad_scale)
                else:
                    ops.adamw_multi(table, len(rows), group["lr"], b1, b2, group["eps"], group["weight_decay"], step,
                                    grad_scale)
            # the kernel writes through raw pointers: tell autograd (and the packed bf16 weight copies keyed on
            # ``_version``, model.py:_Packed) that these parameters changed
            if touched:
                torch.autograd.graph.increment_version(touched)
            by_packs = {}
            for packs, ri in marks:                         # ... and these copies are already those of the new version
                by_packs.setdefault(id(packs), (packs, []))[1].append(ri)
            for packs, idx in by_packs.values():
                packs.mark_current(idx)
        return loss


_EMA_TABLES = {}


@torch.no_grad()
def update_ema_model(ema_model, model, decay):
    """distilled_trainer.py:319-334 without the GPU->CPU round trip (the EMA copy lives in HBM), and as ONE launch for all
    parameters (omh_ema_update_multi) instead of one per tensor; the pointer table is rebuilt only when an address or a
    size changes."""
    rows, touched, keep = [], [], []
    dev = None
    for target, source in zip(ema_model.parameters(), model.parameters()):
        src = source.data
        if src.device != target.device or src.dtype != torch.float32 or not src.is_contiguous():
            src = src.to(device=target.device, dtype=torch.float32).contiguous()
            keep.append(src)
        if target.dtype != torch.float32 or not target.is_contiguous() or target.numel() == 0:
            if target.numel():
                ops.ema_update(target.data, src, decay)             # an odd one out: its own launch
                touched.append(target)
            continue
        dev = target.device
        rows.append((target.data_ptr(), src.data_ptr(), target.numel()))
        touched.append(target)
    if rows:
        key = (id(ema_model), id(model))
        ent = _EMA_TABLES.get(key)
        if ent is None or ent[0] != rows:
            full, chunk0 = [], 0
            for t_, s_, n_ in rows:
                full.append([t_, s_, n_, chunk0])
                chunk0 += (n_ + 4095) // 4096
            ent = _EMA_TABLES[key] = (rows, torch.tensor(full, dtype=torch.int64).to(dev), chunk0)
            if len(_EMA_TABLES) > 8:
                _EMA_TABLES.pop(next(iter(_EMA_TABLES)))
        ops.ema_update_multi(ent[1], len(rows), ent[2], decay)
    if touched:
        torch.autograd.graph.increment_version(touched)
