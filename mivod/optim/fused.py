"""Fused multi-tensor optimizers on flat parameter arenas.

MI355X design: every param group's parameters (per dtype) live in ONE flat,
64-element-aligned arena laid out in *backward order* (reverse registration
order), and each ``Parameter`` is a strided view into it (channels_last
preserved).  Gradients are packed into a flat grad arena of the same layout,
so a gradient bucket is simply a contiguous range ``[lo, hi)`` of the arena and
one kernel launch updates the whole bucket: grad read once, fp32 master and
optimizer state read+written once, the bf16 model copy written in the same
pass.  ``mivod.torch.DistributedOptimizer`` launches that kernel on the comm
stream right after the bucket's RCCL allreduce, overlapped with the rest of
backward.

Reference parity: the optimizers the reference trains with — Keras ``Adadelta``
(/root/reference/mnist_keras.py:84) and ``tf.optimizers.Adam``
(/root/reference/tensorflow2_keras_mnist.py:55) — plus SGD-momentum (ResNet-50)
and LARS (large-batch ResNet), per BASELINE.json north star.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional

import torch

from ..ops import kernels as K

ALIGN = 64  # elements; keeps every slot 16-byte aligned for bf16/fp16/fp32


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def check_max_grad_norm(v):
    """``max_grad_norm`` as a float, or None when clipping is off; a value that is not a
    positive finite number raises."""
    if v is None:
        return None
    f = float(v)
    if not (math.isfinite(f) and f > 0.0):
        raise ValueError(f"max_grad_norm must be a positive finite number or None, not {v!r}")
    return f


def check_ema_decay(v):
    """``ema_decay`` as a float, or None when weight averaging is off; a value outside
    [0, 1) raises."""
    if v is None:
        return None
    f = float(v)
    if not 0.0 <= f < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1) or None, not {v!r}")
    return f


def dyn_values(a) -> List[float]:
    """[lr, first, bc1, bc2] of arena ``a`` for its current ``a.step``: the device
    hyperparameter block of a HIP-graph replay (mivod.torch.graphs)."""
    g = a.group
    bc1 = bc2 = 1.0
    betas = g.get("betas")
    if betas is not None:
        bc1 = 1.0 - float(betas[0]) ** a.step
        bc2 = 1.0 - float(betas[1]) ** a.step
    return [float(g["lr"]), 1.0 if a.step == 1 else 0.0, bc1, bc2]


def _check_adam_ranges(name, lr, betas, eps, weight_decay):
    if not 0.0 <= lr:
        raise ValueError(f"{name}: invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"{name}: invalid epsilon value: {eps}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"{name}: invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"{name}: invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"{name}: invalid weight_decay value: {weight_decay}")


class Arena:
    """A flat arena for the params of one (param_group, dtype)."""

    def __init__(self, group: dict, group_index: int, params: List[torch.nn.Parameter],
                 state_names: List[str], grad_dtype: Optional[torch.dtype] = None):
        assert params
        self.group = group
        self.group_index = group_index
        self.params = params                      # arena (backward) order
        self.dtype = params[0].dtype
        self.device = params[0].device
        self.offsets: List[int] = []
        o = 0
        for p in params:
            if not K.is_dense(p):
                raise ValueError("fused optimizers need dense parameters")
            self.offsets.append(o)
            o += _align(p.numel())
        self.numel = o
        self.index = {id(p): i for i, p in enumerate(params)}
        # model arena: params become views into it
        self.model = torch.zeros(self.numel, dtype=self.dtype, device=self.device)
        with torch.no_grad():
            for p, off in zip(params, self.offsets):
                view = torch.as_strided(self.model, p.size(), p.stride(), off)
                view.copy_(p.data)
                p.data = view
        self.low_precision = self.dtype != torch.float32
        self.master = self.model.float() if self.low_precision else self.model
        self.grad_dtype = grad_dtype or self.dtype
        self.grad = torch.zeros(self.numel, dtype=self.grad_dtype, device=self.device)
        self.state: Dict[str, torch.Tensor] = {
            n: torch.zeros(self.numel, dtype=torch.float32, device=self.device) for n in state_names}
        self.step = 0
        self.versions = [p._version for p in params]
        self.tables: Dict[tuple, K.ChunkTable] = {}
        self.workspace: Dict[str, torch.Tensor] = {}
        self.dyn: Optional[torch.Tensor] = None   # [lr, first, bc1, bc2] for graph replays
        self.ema: Optional[torch.Tensor] = None   # fp32 average of the master (ema_decay)
        self.ema_updates = 0                      # updates counted, the copying first included
        self.ema_counted = False                  # the current step advanced ema_updates

    # -- views ---------------------------------------------------------------
    def slot(self, flat: torch.Tensor, i: int) -> torch.Tensor:
        p = self.params[i]
        return torch.as_strided(flat, p.size(), p.stride(), self.offsets[i])

    def range_of(self, i0: int, i1: int):
        """Element range covering params [i0, i1) (aligned)."""
        lo = self.offsets[i0]
        hi = self.offsets[i1] if i1 < len(self.params) else self.numel
        return lo, hi

    def sync_master_if_modified(self):
        """Params modified in place outside the optimizer (broadcast_parameters,
        load_state_dict, manual edits) re-seed their fp32 master slot."""
        if not self.low_precision:
            return
        for i, p in enumerate(self.params):
            v = p._version
            if v != self.versions[i]:
                lo = self.offsets[i]
                n = p.numel()
                with torch.no_grad():
                    self.master[lo:lo + n].copy_(self.model[lo:lo + n])
                self.versions[i] = v

    def table(self, i0: int, i1: int) -> K.ChunkTable:
        key = (i0, i1)
        t = self.tables.get(key)
        if t is None:
            lo = self.offsets[i0]
            sizes = [self.params[i].numel() for i in range(i0, i1)]
            offs = [self.offsets[i] - lo for i in range(i0, i1)]
            t = K.make_chunk_table(sizes, self.device, offs)
            self.tables[key] = t
        return t


class FusedOptimizer(torch.optim.Optimizer):
    """Base class: arena management, standalone ``step()``, state-dict views.

    ``max_grad_norm`` (every ``Fused*`` constructor takes it; default None = off) clips the
    global L2 norm of the gradient, over all param groups and arenas, to that value before
    the update, as ``torch.nn.utils.clip_grad_norm_`` does: the gradient is scaled by
    min(1, max_grad_norm / (norm + 1e-6)).  The norm, the coefficient and the scaling stay
    on the device (csrc/kernels/mv_clip.hip; the step kernels multiply their gradient scale
    by the coefficient), so there is no host synchronisation, and under
    ``mivod.torch.DistributedOptimizer`` the norm is that of the reduced (averaged) gradient
    with no extra collective.  It is a plain attribute, not part of ``param_groups`` or
    ``state_dict()``, and may be changed or set to None between eager steps; a HIP graph
    keeps the value it was captured with.  ``grad_norm()`` reads the last measured norm.

    ``ema_decay`` (every ``Fused*`` constructor takes it; default None = off) keeps an fp32
    exponential moving average of the fp32 master weights in one more flat arena, 4 bytes per
    parameter, allocated and seeded with the weights at the start of the first step that runs
    with it on: after every update, one streaming pass (csrc/kernels/mv_ema.hip) behind the
    fused step, on the same stream and under the same overflow-guard flag, computes
    ema += (1 - ema_decay) * (w - ema); the first update copies the weights
    (``torch.optim.swa_utils.AveragedModel`` and Keras 3 start there too).  Like
    ``max_grad_norm`` it is a plain attribute that may be changed or set to None between
    eager steps, and a HIP graph keeps the value it was captured with.
    ``ema_parameters()`` evaluates with the average, ``ema_overwrite()`` adopts it, and
    ``state_dict()`` carries it as ``ema_param`` / ``ema_updates`` while it exists.  See
    docs/EMA.md."""

    _state_names: List[str] = []

    def __init__(self, params, defaults, grad_dtype: Optional[torch.dtype] = None,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None):
        super().__init__(params, defaults)
        self._mv_arenas: Optional[List[Arena]] = None
        self._mv_grad_dtype = grad_dtype
        self._mv_external_grads = False   # True when DistributedOptimizer packs grads
        self._mv_graph = False            # True while a HIP graph captures the step
        self._mv_skip = None              # device int32 skip flag (overflow guard)
        self._mv_clip = None              # device fp32 clip coefficient the step kernels read
        self._mv_clip_block = None        # device fp32 [coefficient, norm] of the last step
        self._mv_clip_ws = None           # fp32 sum-of-squares partials, one per 4096 elements
        check_max_grad_norm(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        check_ema_decay(ema_decay)
        self.ema_decay = ema_decay

    # ---- layout ----------------------------------------------------------
    def _mv_build(self, grad_dtype_for=None) -> List[Arena]:
        if self._mv_arenas is not None:
            return self._mv_arenas
        arenas = []
        for gi, g in enumerate(self.param_groups):
            params = [p for p in g["params"] if p.requires_grad]
            by_dtype: Dict[torch.dtype, List[torch.nn.Parameter]] = {}
            for p in reversed(params):                # backward order
                by_dtype.setdefault(p.dtype, []).append(p)
            for dt, ps in by_dtype.items():
                gdt = self._mv_grad_dtype
                if grad_dtype_for is not None:
                    gdt = grad_dtype_for(dt)
                arenas.append(Arena(g, gi, ps, self._state_names, gdt))
        self._mv_arenas = arenas
        self._mv_expose_state()
        return arenas

    def _mv_expose_state(self):
        """Per-param state entries are views into the flat state arenas, so
        ``state_dict()`` / ``broadcast_optimizer_state`` work unchanged."""
        for a in self._mv_arenas:
            for i, p in enumerate(a.params):
                st = self.state[p]
                for n, flat in a.state.items():
                    st[n] = a.slot(flat, i)
                if a.low_precision:
                    st["master_param"] = a.slot(a.master, i)
                if a.ema is not None:
                    st["ema_param"] = a.slot(a.ema, i)
                    st["ema_updates"] = torch.tensor(float(a.ema_updates))
                st["step"] = torch.tensor(float(a.step))

    def _mv_begin_step(self):
        decay = check_ema_decay(self.ema_decay)
        for a in self._mv_build():
            a.sync_master_if_modified()
            a.step += 1
            a.ema_counted = decay is not None
            if a.ema_counted:
                self._mv_ema_arena(a)
                a.ema_updates += 1

    def _mv_uncount_step(self, a: Arena):
        """The step that ``_mv_begin_step`` counted last took no update of ``a`` (the overflow
        guard skipped it): neither the step nor its EMA update is counted."""
        a.step = max(a.step - 1, 0)
        if a.ema_counted:
            a.ema_updates = max(a.ema_updates - 1, 0)
            a.ema_counted = False

    def _mv_end_step(self):
        for a in self._mv_arenas or []:
            a.versions = [p._version for p in a.params]

    def state_dict(self):
        for a in self._mv_arenas or []:
            for p in a.params:
                self.state[p]["step"] = torch.tensor(float(a.step))
                if a.ema is not None:
                    self.state[p]["ema_updates"] = torch.tensor(float(a.ema_updates))
        return super().state_dict()

    # ---- the fp32 moving average of the master weights ----------------------
    def _mv_ema_arena(self, a: Arena) -> torch.Tensor:
        """The arena's fp32 EMA, allocated on first use and seeded with the master."""
        if a.ema is None:
            if self._mv_graph:
                raise RuntimeError("ema_decay must be set before make_graphed_step's eager "
                                   "warmup: a HIP-graph capture cannot allocate the EMA arena")
            a.ema = a.master.clone()
            a.ema_updates = 0
            self._mv_expose_state()
        return a.ema

    def _mv_apply_ema(self, a: Arena, i0: int, i1: int):
        """The EMA update of params [i0, i1) of ``a``, right behind their fused step: same
        stream, same skip flag.  The arena's first counted update copies the weights."""
        decay = check_ema_decay(self.ema_decay)
        if decay is None or not a.ema_counted:
            return
        if a.ema_updates <= 1:
            if self._mv_graph:
                raise RuntimeError("a HIP-graph capture needs an eager step with ema_decay set "
                                   "before it (the copying first EMA update)")
            decay = 0.0
        lo, hi = a.range_of(i0, i1)
        K.ema_update(a.master[lo:hi], a.ema[lo:hi], decay=decay, skip=self._mv_skip)

    def _mv_ema_sync(self):
        """Hook of DistributedOptimizer: refuse inside a step, order after the comm stream."""

    @contextlib.contextmanager
    def ema_parameters(self):
        """Context manager: inside it the parameters (fp32 master, low-precision model copy
        and therefore every parameter view) hold the moving average; on exit the training
        weights are back bit for bit (the exchange is exact).  Do not step inside it."""
        arenas = [a for a in self._mv_build() if a.ema is not None]
        if not arenas:
            raise RuntimeError("ema_parameters(): no step has run with ema_decay set")
        self._mv_ema_sync()
        for a in self._mv_arenas:
            a.sync_master_if_modified()
        self._mv_ema_exchange(arenas)
        try:
            yield self
        finally:
            self._mv_ema_sync()
            self._mv_ema_exchange(arenas)

    @torch.no_grad()
    def _mv_ema_exchange(self, arenas):
        for a in arenas:
            K.ema_swap(a.master, a.ema, a.model if a.low_precision else None)
            a.versions = [p._version for p in a.params]

    @torch.no_grad()
    def ema_overwrite(self):
        """Adopt the moving average as the training weights: master = ema, model copy =
        cast(ema).  The average itself is untouched."""
        arenas = [a for a in self._mv_build() if a.ema is not None]
        if not arenas:
            raise RuntimeError("ema_overwrite(): no step has run with ema_decay set")
        self._mv_ema_sync()
        for a in arenas:
            a.sync_master_if_modified()
            K.ema_overwrite(a.master, a.ema, a.model if a.low_precision else None)
            a.versions = [p._version for p in a.params]

    @torch.no_grad()
    def _mv_adopt_ema(self, updates: int):
        """Per-parameter ``ema_param`` entries that a loader other than ``load_state_dict``
        put into ``self.state`` (mivod.kerasfw.load_model) become the arenas' average."""
        for a in self._mv_build():
            saved = [self.state[p].get("ema_param") for p in a.params]
            if a.ema is None and all(torch.is_tensor(t) for t in saved):
                a.ema = a.master.clone()
                for i, t in enumerate(saved):
                    a.slot(a.ema, i).copy_(t)
                a.ema_updates = int(updates)
        self._mv_expose_state()

    # ---- the fused update of a bucket ------------------------------------
    def _mv_apply(self, a: Arena, i0: int, i1: int, gscale: float = 1.0):
        raise NotImplementedError

    def _mv_dyn(self, a: Arena):
        """Device hyperparameter block for graph capture (None in eager mode)."""
        if not self._mv_graph:
            return None
        if a.dyn is None:
            a.dyn = torch.zeros(4, dtype=torch.float32, device=a.device)
        return a.dyn

    def _mv_dyn_values(self, a: Arena) -> List[float]:
        """The four floats a HIP-graph replay writes into ``a.dyn`` before it launches, for
        the arena's current ``a.step``: [lr, first, bc1, bc2] unless the optimizer's kernel
        reads its block differently."""
        return dyn_values(a)

    def _mv_slices(self, a: Arena, i0: int, i1: int):
        lo, hi = a.range_of(i0, i1)
        model = a.model[lo:hi] if a.low_precision else None
        st = {n: f[lo:hi] for n, f in a.state.items()}
        return a.grad[lo:hi], a.master[lo:hi], st, model

    # ---- global gradient-norm clipping ------------------------------------
    def _mv_clip_buffers(self, device, nchunks: int):
        """The device block [coefficient, norm] and a partial workspace of at least
        ``nchunks`` entries (kept: a captured HIP graph holds their addresses)."""
        blk = self._mv_clip_block
        if blk is None or blk.device != device:
            blk = self._mv_clip_block = torch.tensor([1.0, 0.0], dtype=torch.float32,
                                                     device=device)
        ws = self._mv_clip_ws
        if ws is None or ws.device != device or ws.numel() < nchunks:
            ws = self._mv_clip_ws = torch.empty(max(nchunks, 1), dtype=torch.float32,
                                                device=device)
        return blk, ws

    def grad_norm(self) -> torch.Tensor:
        """The global L2 norm of the last clipped step's gradient before clipping (under
        DistributedOptimizer: of the averaged gradient), a 0-dim device tensor.  No host
        synchronisation happens here; ``.item()`` is the caller's."""
        if self._mv_clip_block is None:
            raise RuntimeError("grad_norm(): no step has run with max_grad_norm set")
        return self._mv_clip_block[1].clone()

    # ---- standalone step (no DistributedOptimizer) -------------------------
    def _mv_pack_local(self, a: Arena):
        """p.grad of every parameter of ``a`` -> its slot of the flat gradient arena."""
        grads, offs = [], []
        for i, p in enumerate(a.params):
            if p.grad is None:
                lo = a.offsets[i]
                a.grad[lo:lo + p.numel()].zero_()
                continue
            g = p.grad
            if g.stride() != p.stride():
                g = torch.empty_like(p).copy_(g)
            grads.append(g)
            offs.append(a.offsets[i])
        by_dt: Dict[torch.dtype, tuple] = {}
        for g, o in zip(grads, offs):
            by_dt.setdefault(g.dtype, ([], []))
            by_dt[g.dtype][0].append(g)
            by_dt[g.dtype][1].append(o)
        for gl, ol in by_dt.values():
            K.pack(gl, a.grad, ol)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        arenas = self._mv_build()
        self._mv_begin_step()
        max_norm = check_max_grad_norm(self.max_grad_norm)
        if max_norm is None:
            for a in arenas:
                if not self._mv_external_grads:
                    self._mv_pack_local(a)
                self._mv_apply(a, 0, len(a.params), 1.0)
                self._mv_apply_ema(a, 0, len(a.params))
        elif arenas:
            # every arena packed and measured before the first update: the coefficient is
            # global.  The alignment gaps of an arena are zeros, so its whole range is summed.
            if not self._mv_external_grads:
                for a in arenas:
                    self._mv_pack_local(a)
            counts = [K.sumsq_chunks(a.numel) for a in arenas]
            blk, ws = self._mv_clip_buffers(arenas[0].device, sum(counts))
            o = 0
            for a, c in zip(arenas, counts):
                K.grad_sumsq(a.grad, ws[o:o + c])
                o += c
            K.clip_finalize(ws, o, blk, gscale=1.0, max_norm=max_norm)
            self._mv_clip = blk[0:1]
            try:
                for a in arenas:
                    self._mv_apply(a, 0, len(a.params), 1.0)
                    self._mv_apply_ema(a, 0, len(a.params))
            finally:
                self._mv_clip = None
        self._mv_end_step()
        return loss

    def load_state_dict(self, state_dict):
        arenas = self._mv_build()
        # torch's loader casts every floating state tensor to its parameter's dtype
        # (bf16 for a bf16 model): take the exact fp32 values (master weights, Adam
        # moments) from the incoming dict instead of from the cast copies
        raw = {}
        for g_saved, g_live in zip(state_dict.get("param_groups", []), self.param_groups):
            for k, p in zip(g_saved["params"], g_live["params"]):
                if k in state_dict.get("state", {}):
                    raw[p] = state_dict["state"][k]
        super().load_state_dict(state_dict)
        # a torch.optim state dict brings torch's group keys: ours that it lacks keep their
        # constructor values
        for g in self.param_groups:
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        # torch replaced our views with fresh tensors: copy them back into the arenas
        with torch.no_grad():
            for a in arenas:
                steps, emas = [], []
                for i, p in enumerate(a.params):
                    st = raw.get(p) or self.state.get(p, {})
                    if "ema_param" in st and "ema_updates" in st:
                        emas.append((i, st["ema_param"], float(st["ema_updates"])))
                    for n, flat in a.state.items():
                        if n in st and torch.is_tensor(st[n]):
                            a.slot(flat, i).copy_(st[n])
                    if a.low_precision:
                        if "master_param" in st:
                            a.slot(a.master, i).copy_(st["master_param"])
                        else:
                            a.slot(a.master, i).copy_(p.data)
                    if "step" in st:
                        steps.append(float(st["step"]))
                if steps:
                    a.step = int(max(steps))
                a.versions = [p._version for p in a.params]
                if len(emas) == len(a.params):
                    # the exact fp32 average, as master_param above
                    if a.ema is None:
                        a.ema = a.master.clone()
                    for i, e, _ in emas:
                        a.slot(a.ema, i).copy_(e)
                    a.ema_updates = int(max(n for _, _, n in emas))
                else:
                    # a dict without the average: the next step with ema_decay set seeds a
                    # new one from the weights it finds
                    a.ema = None
                    a.ema_updates = 0
                a.ema_counted = False
        # entries torch copied from a dict that this optimizer does not keep
        for st in self.state.values():
            st.pop("ema_param", None)
            st.pop("ema_updates", None)
        self._mv_expose_state()

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)


class FusedSGD(FusedOptimizer):
    """SGD with momentum / dampening / nesterov / weight decay (torch.optim.SGD
    semantics, momentum buffer seeded with the first gradient)."""

    def __init__(self, params, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._state_names = ["momentum_buffer"] if momentum != 0 else []
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov), grad_dtype,
                         max_grad_norm, ema_decay)

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        K.sgd_step(g, w, st.get("momentum_buffer"), model, lr=hp["lr"], momentum=hp["momentum"],
                   dampening=hp["dampening"], weight_decay=hp["weight_decay"], gscale=gscale,
                   nesterov=hp["nesterov"], first=(a.step == 1), dyn=self._mv_dyn(a),
                   skip=self._mv_skip, gclip=self._mv_clip)


class FusedAdam(FusedOptimizer):
    """Adam / AdamW.  ``keras_eps=True`` uses Keras' epsilon placement
    (eps scaled by sqrt(1-beta2^t)), matching tf.optimizers.Adam.

    ``amsgrad=True`` keeps the running maximum of the second moment in a third state stream,
    ``max_exp_avg_sq`` (torch's name, so a ``torch.optim.Adam(amsgrad=True)`` state dict
    loads), and divides by it: the maximum is taken on the uncorrected moment, as torch and
    Keras take it.  It decides which state arenas exist, so it is fixed at construction; the
    ``amsgrad`` entry of a param group is informational."""

    _state_names = ["exp_avg", "exp_avg_sq"]

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 adamw=False, keras_eps=False, grad_dtype=None, max_grad_norm=None,
                 amsgrad=False, ema_decay=None):
        _check_adam_ranges(type(self).__name__, lr, betas, eps, weight_decay)
        self._mv_amsgrad = bool(amsgrad)
        if self._mv_amsgrad:
            self._state_names = ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      adamw=adamw, keras_eps=keras_eps,
                                      amsgrad=self._mv_amsgrad),
                         grad_dtype, max_grad_norm, ema_decay)

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        b1, b2 = hp["betas"]
        kw = dict(lr=hp["lr"], beta1=b1, beta2=b2, eps=hp["eps"], weight_decay=hp["weight_decay"],
                  gscale=gscale, step=a.step, adamw=hp["adamw"], keras_eps=hp["keras_eps"],
                  dyn=self._mv_dyn(a), skip=self._mv_skip, gclip=self._mv_clip)
        if self._mv_amsgrad:
            K.adam_amsgrad_step(g, w, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"], model,
                                **kw)
        else:
            K.adam_step(g, w, st["exp_avg"], st["exp_avg_sq"], model, **kw)


class FusedAdamW(FusedAdam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 grad_dtype=None, max_grad_norm=None, amsgrad=False, ema_decay=None):
        super().__init__(params, lr, betas, eps, weight_decay, adamw=True, grad_dtype=grad_dtype,
                         max_grad_norm=max_grad_norm, amsgrad=amsgrad, ema_decay=ema_decay)


class FusedAdadelta(FusedOptimizer):
    """Adadelta (Zeiler 2012; torch / Keras semantics — Keras uses eps=1e-7)."""

    _state_names = ["square_avg", "acc_delta"]

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0, grad_dtype=None,
                 max_grad_norm=None, ema_decay=None):
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay),
                         grad_dtype, max_grad_norm, ema_decay)

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        K.adadelta_step(g, w, st["square_avg"], st["acc_delta"], model, lr=hp["lr"], rho=hp["rho"],
                        eps=hp["eps"], weight_decay=hp["weight_decay"], gscale=gscale,
                        dyn=self._mv_dyn(a), skip=self._mv_skip, gclip=self._mv_clip)


class FusedLARS(FusedOptimizer):
    """LARS (You, Gitman, Ginsburg 2017) with momentum.  Parameters with
    ``dim() <= 1`` (BN affine, biases) are excluded from adaptation and weight
    decay when ``exclude_1d=True`` (the common large-batch ResNet recipe)."""

    _state_names = ["momentum_buffer"]

    def __init__(self, params, lr=0.1, momentum=0.9, weight_decay=1e-4, eta=0.001, eps=0.0,
                 exclude_1d=True, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, eta=eta,
                                      eps=eps, exclude_1d=exclude_1d),
                         grad_dtype, max_grad_norm, ema_decay)
        self._mv_flags: Dict[tuple, torch.Tensor] = {}

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        key = (id(a), i0, i1)
        flags = self._mv_flags.get(key)
        if flags is None:
            fl = [1 if (hp["exclude_1d"] and a.params[i].dim() <= 1) else 0 for i in range(i0, i1)]
            flags = self._mv_flags[key] = torch.tensor(fl, dtype=torch.int32, device=a.device)
        K.lars_step(g, w, st["momentum_buffer"], model, a.table(i0, i1), flags, lr=hp["lr"],
                    momentum=hp["momentum"], weight_decay=hp["weight_decay"], eta=hp["eta"],
                    gscale=gscale, eps=hp["eps"], first=(a.step == 1), workspace=a.workspace,
                    dyn=self._mv_dyn(a), skip=self._mv_skip, gclip=self._mv_clip)


class FusedLAMB(FusedOptimizer):
    """LAMB (You et al. 2019, arXiv 1904.00962): Adam moments with bias correction and
    decoupled weight decay inside the update direction, scaled per parameter tensor by the
    trust ratio |w| / |u|.  Parameters with ``dim() <= 1`` (biases, LayerNorm) take no
    weight decay and trust 1 when ``exclude_1d=True``; with ``exclude_1d=False`` every
    tensor is adapted and decayed.

    ``max_grad_norm`` clips the global gradient norm before the moments are updated (the
    BERT pre-training recipe; see ``FusedOptimizer``): every bucket is reduced and measured
    before the first update, so under DistributedOptimizer the updates are not overlapped
    with backward while it is set.

    Not provided: trust-ratio clamping, ``grad_averaging=False`` and an ``always_adapt``
    switch."""

    _state_names = ["exp_avg", "exp_avg_sq"]

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 exclude_1d=True, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      exclude_1d=exclude_1d), grad_dtype, max_grad_norm, ema_decay)
        self._mv_flags: Dict[tuple, torch.Tensor] = {}

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        key = (id(a), i0, i1)
        flags = self._mv_flags.get(key)
        if flags is None:
            fl = [1 if (hp["exclude_1d"] and a.params[i].dim() <= 1) else 0 for i in range(i0, i1)]
            flags = self._mv_flags[key] = torch.tensor(fl, dtype=torch.int32, device=a.device)
        b1, b2 = hp["betas"]
        K.lamb_step(g, w, st["exp_avg"], st["exp_avg_sq"], model, a.table(i0, i1), flags,
                    lr=hp["lr"], beta1=b1, beta2=b2, eps=hp["eps"],
                    weight_decay=hp["weight_decay"], gscale=gscale, step=a.step,
                    workspace=a.workspace, dyn=self._mv_dyn(a), skip=self._mv_skip,
                    gclip=self._mv_clip)


class FusedRMSprop(FusedOptimizer):
    """RMSprop with torch.optim.RMSprop's semantics and state names (``square_avg``,
    ``momentum_buffer`` when ``momentum != 0``, ``grad_avg`` when ``centered``), so a
    torch.optim.RMSprop state dict loads.  One deviation: the centered variance
    ``square_avg - grad_avg^2`` is clamped at zero before the root (rounded, it can fall
    below zero, where torch produces NaN).  ``momentum`` and ``centered`` decide which state
    arenas exist, so they are fixed at construction; a group's momentum may change between
    non-zero values."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0,
                 centered=False, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        if lr < 0 or eps < 0 or alpha < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedRMSprop: lr, alpha, eps, momentum and weight_decay must be >= 0")
        self._state_names = (["square_avg"] + (["momentum_buffer"] if momentum != 0 else [])
                             + (["grad_avg"] if centered else []))
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay,
                                      momentum=momentum, centered=bool(centered)), grad_dtype,
                         max_grad_norm, ema_decay)

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        K.rmsprop_step(g, w, st["square_avg"], st.get("grad_avg"), st.get("momentum_buffer"), model,
                       lr=hp["lr"], alpha=hp["alpha"], eps=hp["eps"],
                       weight_decay=hp["weight_decay"], momentum=hp["momentum"],
                       centered=hp["centered"], gscale=gscale, dyn=self._mv_dyn(a),
                       skip=self._mv_skip, gclip=self._mv_clip)


class FusedAdagrad(FusedOptimizer):
    """Adagrad with torch.optim.Adagrad's semantics and state name (``sum``, filled with
    ``initial_accumulator_value`` when the arenas are built).  The decayed rate
    lr / (1 + (step-1) lr_decay) is taken on the host, so a captured HIP graph, whose device
    hyperparameter block carries the rate but no step count, refuses ``lr_decay != 0``."""

    _state_names = ["sum"]

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0,
                 eps=1e-10, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        if lr < 0 or lr_decay < 0 or weight_decay < 0 or initial_accumulator_value < 0 or eps < 0:
            raise ValueError("FusedAdagrad: lr, lr_decay, weight_decay, "
                             "initial_accumulator_value and eps must be >= 0")
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                                      initial_accumulator_value=initial_accumulator_value),
                         grad_dtype, max_grad_norm, ema_decay)

    def _mv_build(self, grad_dtype_for=None):
        if self._mv_arenas is None:
            # the alignment gaps hold the value too: their gradients are zero, so they stay put
            for a in super()._mv_build(grad_dtype_for):
                a.state["sum"].fill_(float(a.group["initial_accumulator_value"]))
        return self._mv_arenas

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        if hp["lr_decay"] != 0 and self._mv_graph:
            raise NotImplementedError(
                "FusedAdagrad: lr_decay != 0 under HIP-graph capture (the replayed "
                "hyperparameter block carries lr but no step count)")
        clr = hp["lr"] / (1.0 + (a.step - 1) * hp["lr_decay"])
        K.adagrad_step(g, w, st["sum"], model, lr=clr, eps=hp["eps"],
                       weight_decay=hp["weight_decay"], gscale=gscale, dyn=self._mv_dyn(a),
                       skip=self._mv_skip, gclip=self._mv_clip)


class FusedAdamax(FusedOptimizer):
    """Adamax (Kingma & Ba 2015, section 7) with torch.optim.Adamax's semantics and state names
    (``exp_avg``, ``exp_inf``), so a torch.optim.Adamax state dict loads: with
    gr = g + weight_decay * w, exp_avg = b1 exp_avg + (1-b1) gr,
    exp_inf = max(b2 exp_inf, |gr| + eps) and w -= lr / (1 - b1^t) * exp_avg / exp_inf.
    ``keras_eps=True`` uses Keras' epsilon placement: exp_inf = max(b2 exp_inf, |gr|) and the
    divisor exp_inf + eps.  Weight decay is the coupled one only.  One deviation from torch:
    an element whose divisor is exactly 0 (``eps=0`` and a gradient history of zeros) takes no
    update, where torch divides 0 by 0 and stores NaN."""

    _state_names = ["exp_avg", "exp_inf"]

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 keras_eps=False, grad_dtype=None, max_grad_norm=None, ema_decay=None):
        _check_adam_ranges("FusedAdamax", lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      keras_eps=bool(keras_eps)),
                         grad_dtype, max_grad_norm, ema_decay)

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        b1, b2 = hp["betas"]
        K.adamax_step(g, w, st["exp_avg"], st["exp_inf"], model, lr=hp["lr"], beta1=b1, beta2=b2,
                      eps=hp["eps"], weight_decay=hp["weight_decay"], gscale=gscale, step=a.step,
                      keras_eps=hp["keras_eps"], dyn=self._mv_dyn(a), skip=self._mv_skip,
                      gclip=self._mv_clip)


class FusedNAdam(FusedOptimizer):
    """NAdam (Dozat 2016) with torch.optim.NAdam's semantics and state names (``exp_avg``,
    ``exp_avg_sq``), which is also Keras ``Nadam``'s rule: with
    mu_t = b1 (1 - 0.5 * 0.96^(t * momentum_decay)) and P_t = mu_1 ... mu_t,
    w -= lr (1-mu_t)/(1-P_t) gr / denom + lr mu_{t+1}/(1 - P_t mu_{t+1}) exp_avg / denom,
    denom = sqrt(exp_avg_sq / (1 - b2^t)) + eps.  ``decoupled_weight_decay=True`` decays the
    weights by 1 - lr * weight_decay instead of adding weight_decay * w to the gradient.

    The two weights and the bias correction are taken on the host in double and handed to the
    kernel (or, under a captured HIP graph, written into its device block [lr, cg, cm, bc2]).
    P_t is not stored: it is derived from the arena's step count and the group's CURRENT
    ``betas[0]`` and ``momentum_decay`` (cached incrementally), so ``load_state_dict`` and a
    graph capture's rollback of the step count need nothing more.  The consequence: a ``beta1``
    or ``momentum_decay`` changed in the middle of training re-derives the whole product with
    the new value, where torch keeps the product of the values each step was taken with.
    ``state_dict()`` exposes the product per parameter as ``mu_product``, torch's entry; on
    loading it is ignored in favour of the derived one."""

    _state_names = ["exp_avg", "exp_avg_sq"]

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 momentum_decay=4e-3, decoupled_weight_decay=False, grad_dtype=None,
                 max_grad_norm=None, ema_decay=None):
        _check_adam_ranges("FusedNAdam", lr, betas, eps, weight_decay)
        if not 0.0 <= momentum_decay:
            raise ValueError(f"FusedNAdam: invalid momentum_decay value: {momentum_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      momentum_decay=momentum_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)),
                         grad_dtype, max_grad_norm, ema_decay)
        self._mv_mu_key = None
        self._mv_mu_products = [1.0]      # P_0 .. P_t for _mv_mu_key = (beta1, momentum_decay)

    def mu_product(self, step: int, beta1: float, momentum_decay: float) -> float:
        """P_step = mu_1 ... mu_step (1 at step 0), in double."""
        key = (float(beta1), float(momentum_decay))
        if key != self._mv_mu_key:
            self._mv_mu_key, self._mv_mu_products = key, [1.0]
        ps = self._mv_mu_products
        while len(ps) <= step:
            ps.append(ps[-1] * K.nadam_mu(len(ps), *key))
        return ps[step]

    def _mv_coefficients(self, a):
        """(cg, cm, bc2) of the step the arena's counter stands at."""
        hp = a.group
        b1, b2 = (float(b) for b in hp["betas"])
        md = float(hp["momentum_decay"])
        cg, cm = K.nadam_coefficients(K.nadam_mu(a.step, b1, md), K.nadam_mu(a.step + 1, b1, md),
                                      self.mu_product(a.step, b1, md))
        return cg, cm, 1.0 - b2 ** a.step

    def _mv_dyn_values(self, a):
        cg, cm, bc2 = self._mv_coefficients(a)
        return [float(a.group["lr"]), cg, cm, bc2]

    def state_dict(self):
        for a in self._mv_arenas or []:
            p_t = self.mu_product(a.step, float(a.group["betas"][0]),
                                  float(a.group["momentum_decay"]))
            for p in a.params:
                self.state[p]["mu_product"] = torch.tensor(p_t)
        return super().state_dict()

    def _mv_apply(self, a, i0, i1, gscale=1.0):
        g, w, st, model = self._mv_slices(a, i0, i1)
        hp = a.group
        b1, b2 = hp["betas"]
        cg, cm, bc2 = self._mv_coefficients(a)
        K.nadam_step(g, w, st["exp_avg"], st["exp_avg_sq"], model, lr=hp["lr"], cg=cg, cm=cm,
                     bc2=bc2, beta1=b1, beta2=b2, eps=hp["eps"], weight_decay=hp["weight_decay"],
                     gscale=gscale, adamw=hp["decoupled_weight_decay"], dyn=self._mv_dyn(a),
                     skip=self._mv_skip, gclip=self._mv_clip)
