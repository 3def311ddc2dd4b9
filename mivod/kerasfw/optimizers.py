"""Keras optimizers on mivod's fused flat-arena optimizers.

Keras semantics (keras 2.x / tf.keras): ``lr`` / ``learning_rate`` and
``momentum`` are backend Variables that callbacks mutate with
``K.set_value``; ``get_gradients(loss, params)`` is the hook point horovod's
Keras ``DistributedOptimizer`` overrides (/root/reference/tensorflow2_keras_mnist.py:60-65
explains why the reference must keep Keras on that path); ``get_config`` /
``from_config`` drive re-instantiation and ``load_model``.

The update itself is a mivod fused kernel (FusedAdadelta / FusedAdam with
Keras epsilon placement, amsgrad included / FusedSGD / FusedRMSprop / FusedAdagrad /
FusedAdamax with Keras epsilon placement / FusedNAdam): one launch
per arena on the GPU, the plain-PyTorch reference math on the CPU.  RMSprop and
Adagrad keep torch's form (epsilon outside the root; RMSprop's rate outside its
momentum buffer): see their docstrings for what that changes against tf.keras.

``use_ema`` / ``ema_momentum`` / ``ema_overwrite_frequency`` (tf.keras's names, taken by
every optimizer) keep an fp32 exponential moving average of the trainable variables on the
fused path (``ema_decay`` of the Fused* optimizers, docs/EMA.md).  As in Keras only the
variables the optimizer updates are averaged: BatchNorm's moving mean and variance are not.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .backend import Variable, epsilon


class Optimizer:
    _hyper: tuple = ()

    def __init__(self, name: Optional[str] = None, **kwargs):
        lr = kwargs.pop("learning_rate", None)
        if lr is None:
            lr = kwargs.pop("lr", self._default_lr)
        else:
            kwargs.pop("lr", None)
        self.lr = Variable(lr, "lr")
        self.decay = float(kwargs.pop("decay", 0.0))
        self.clipnorm = kwargs.pop("clipnorm", None)
        self.clipvalue = kwargs.pop("clipvalue", None)
        self.use_ema = bool(kwargs.pop("use_ema", False))
        self.ema_momentum = float(kwargs.pop("ema_momentum", 0.99))
        self.ema_overwrite_frequency = kwargs.pop("ema_overwrite_frequency", None)
        if self.use_ema:
            if not 0.0 <= self.ema_momentum < 1.0:
                raise ValueError(f"ema_momentum must be in [0, 1), not {self.ema_momentum}")
            f = self.ema_overwrite_frequency
            if f is not None and (not isinstance(f, int) or f < 1):
                raise ValueError("ema_overwrite_frequency must be an integer >= 1 or None, "
                                 f"not {f!r}")
        self._name = name or type(self).__name__
        self.iterations = 0
        self._impl = None
        self._params: List[torch.nn.Parameter] = []

    _default_lr = 0.01

    @property
    def learning_rate(self):
        return self.lr

    # -- horovod hook point ------------------------------------------------
    def get_gradients(self, loss, params):
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params)]
        if self.clipnorm is not None:
            norm = torch.sqrt(sum((g.float() ** 2).sum() for g in grads))
            scale = torch.clamp(self.clipnorm / (norm + 1e-12), max=1.0)
            grads = [g * scale for g in grads]
        if self.clipvalue is not None:
            grads = [g.clamp(-self.clipvalue, self.clipvalue) for g in grads]
        return grads

    def _make_impl(self, params):
        raise NotImplementedError

    @property
    def _ema_decay(self):
        """``ema_decay`` of the fused optimizer: ``ema_momentum`` with ``use_ema``, else None."""
        return self.ema_momentum if self.use_ema else None

    def _sync_hyper(self):
        lr = float(self.lr)
        if self.decay:
            lr = lr / (1.0 + self.decay * self.iterations)
        for g in self._impl.param_groups:
            g["lr"] = lr
            if hasattr(self, "momentum") and "momentum" in g:
                g["momentum"] = float(self.momentum)

    def apply_gradients(self, grads_and_vars):
        gv = list(grads_and_vars)
        params = [v for _, v in gv]
        if self._impl is None:
            self._params = params
            self._impl = self._make_impl(params)
        with torch.no_grad():
            for g, p in gv:
                p.grad = g
        self._sync_hyper()
        self._impl.step()
        for p in params:
            p.grad = None
        self.iterations += 1
        if self.use_ema and self.ema_overwrite_frequency and \
                self.iterations % self.ema_overwrite_frequency == 0:
            self._impl.ema_overwrite()

    def finalize_variable_values(self, var_list=None):
        """With ``use_ema``: the variables take their moving average (tf.keras calls this at
        the end of ``fit`` when no ``ema_overwrite_frequency`` is given).  Every variable the
        optimizer updates is overwritten; ``var_list`` is accepted for parity."""
        if self.use_ema and self._impl is not None:
            self._impl.ema_overwrite()

    def minimize(self, loss, var_list):
        self.apply_gradients(zip(self.get_gradients(loss, var_list), var_list))

    # -- Keras config / weights --------------------------------------------
    def get_config(self) -> dict:
        cfg = {"name": self._name, "learning_rate": float(self.lr), "decay": self.decay}
        for h in self._hyper:
            v = getattr(self, h)
            cfg[h] = float(v) if isinstance(v, Variable) else v
        if self.use_ema:
            cfg.update(use_ema=True, ema_momentum=self.ema_momentum,
                       ema_overwrite_frequency=self.ema_overwrite_frequency)
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def variables(self) -> List[torch.Tensor]:
        out = []
        if self._impl is not None:
            for p in self._params:
                st = self._impl.state.get(p, {})
                out.extend(v for k, v in sorted(st.items()) if torch.is_tensor(v) and v.dim() > 0)
        return out

    weights = property(variables)

    def get_weights(self):
        return [self.iterations] + [v.detach().cpu().numpy() for v in self.variables()]

    def state_dict(self):
        return {"iterations": self.iterations, "lr": float(self.lr),
                "impl": self._impl.state_dict() if self._impl is not None else None}

    def load_state_dict(self, sd, params=None):
        self.iterations = int(sd.get("iterations", 0))
        if sd.get("impl") is not None:
            if self._impl is None:
                if params is None:
                    self._pending_state = sd["impl"]
                    return
                self._params = list(params)
                self._impl = self._make_impl(self._params)
            self._impl.load_state_dict(sd["impl"])

    def _maybe_load_pending(self):
        st = getattr(self, "_pending_state", None)
        if st is not None and self._impl is not None:
            self._impl.load_state_dict(st)
            self._pending_state = None


class SGD(Optimizer):
    _default_lr = 0.01
    _hyper = ("momentum", "nesterov")

    def __init__(self, lr=None, momentum=0.0, decay=0.0, nesterov=False, name=None, **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.momentum = Variable(momentum, "momentum")
        self.nesterov = bool(nesterov)

    def _make_impl(self, params):
        from ..optim import FusedSGD
        return FusedSGD(params, lr=float(self.lr), momentum=float(self.momentum) or 0.0,
                        nesterov=self.nesterov, ema_decay=self._ema_decay)

    def _sync_hyper(self):
        super()._sync_hyper()


class Adam(Optimizer):
    _default_lr = 0.001
    _hyper = ("beta_1", "beta_2", "epsilon", "amsgrad")

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False,
                 name=None, **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = float(epsilon if epsilon is not None else 1e-7)
        self.amsgrad = bool(amsgrad)

    def _make_impl(self, params):
        from ..optim import FusedAdam
        return FusedAdam(params, lr=float(self.lr), betas=(self.beta_1, self.beta_2),
                         eps=self.epsilon, keras_eps=True, amsgrad=self.amsgrad,
                         ema_decay=self._ema_decay)


class Adamax(Optimizer):
    """Adamax on ``FusedAdamax`` with Keras' epsilon placement: the infinity norm is
    max(beta_2 u, |g|) and epsilon joins it in the divisor."""
    _default_lr = 0.002
    _hyper = ("beta_1", "beta_2", "epsilon")

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, name=None,
                 **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = float(epsilon if epsilon is not None else 1e-7)

    def _make_impl(self, params):
        from ..optim import FusedAdamax
        return FusedAdamax(params, lr=float(self.lr), betas=(self.beta_1, self.beta_2),
                           eps=self.epsilon, keras_eps=True, ema_decay=self._ema_decay)


class Nadam(Optimizer):
    """Nadam on ``FusedNAdam`` (torch.optim.NAdam's rule, which is Keras 2's):
    ``schedule_decay`` is its ``momentum_decay``."""
    _default_lr = 0.002
    _hyper = ("beta_1", "beta_2", "epsilon", "schedule_decay")

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, schedule_decay=0.004,
                 decay=0.0, name=None, **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = float(epsilon if epsilon is not None else 1e-7)
        self.schedule_decay = float(schedule_decay)

    def _make_impl(self, params):
        from ..optim import FusedNAdam
        return FusedNAdam(params, lr=float(self.lr), betas=(self.beta_1, self.beta_2),
                          eps=self.epsilon, momentum_decay=self.schedule_decay,
                          ema_decay=self._ema_decay)


class Adadelta(Optimizer):
    _default_lr = 1.0
    _hyper = ("rho", "epsilon")

    def __init__(self, lr=None, rho=0.95, epsilon=None, decay=0.0, name=None, **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.rho = float(rho)
        self.epsilon = float(epsilon if epsilon is not None else epsilon_default())

    def _make_impl(self, params):
        from ..optim import FusedAdadelta
        return FusedAdadelta(params, lr=float(self.lr), rho=self.rho, eps=self.epsilon,
                             ema_decay=self._ema_decay)


def epsilon_default():
    return epsilon()


class RMSprop(Optimizer):
    """RMSprop on ``FusedRMSprop`` (torch.optim.RMSprop semantics): ``rho`` is the decay of the
    squared-gradient average and ``epsilon`` is added outside the root, which with the defaults
    is what tf.keras computes up to the placement of epsilon.  With ``momentum > 0`` the form
    differs from tf.keras: there the buffer accumulates ``lr * g / sqrt(avg + epsilon)`` (the
    rate inside the buffer, epsilon inside the root); here it accumulates
    ``g / (sqrt(avg) + epsilon)`` and the rate multiplies the buffer, so a rate changed during
    training rescales the steps already accumulated.  ``momentum`` and ``centered`` are fixed
    once the first step has built the optimizer state."""
    _default_lr = 0.001
    _hyper = ("rho", "epsilon", "momentum", "centered")

    def __init__(self, lr=None, rho=0.9, epsilon=None, decay=0.0, momentum=0.0, centered=False,
                 name=None, **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.rho = float(rho)
        self.epsilon = float(epsilon if epsilon is not None else 1e-7)
        self.momentum = Variable(momentum, "momentum")
        self.centered = bool(centered)

    def _make_impl(self, params):
        from ..optim import FusedRMSprop
        return FusedRMSprop(params, lr=float(self.lr), alpha=self.rho, eps=self.epsilon,
                            momentum=float(self.momentum) or 0.0, centered=self.centered,
                            ema_decay=self._ema_decay)


class Adagrad(Optimizer):
    """Adagrad on ``FusedAdagrad``; ``decay`` is the base class's rate decay
    lr / (1 + decay * iterations), the same schedule as torch's ``lr_decay``."""
    _default_lr = 0.001
    _hyper = ("initial_accumulator_value", "epsilon")

    def __init__(self, lr=None, initial_accumulator_value=0.1, epsilon=None, decay=0.0, name=None,
                 **kw):
        kw.setdefault("lr", lr if lr is not None else self._default_lr)
        super().__init__(name=name, decay=decay, **kw)
        self.initial_accumulator_value = float(initial_accumulator_value)
        self.epsilon = float(epsilon if epsilon is not None else 1e-7)

    def _make_impl(self, params):
        from ..optim import FusedAdagrad
        return FusedAdagrad(params, lr=float(self.lr), eps=self.epsilon,
                            initial_accumulator_value=self.initial_accumulator_value,
                            ema_decay=self._ema_decay)


OPTIMIZERS = {"SGD": SGD, "Adam": Adam, "Adadelta": Adadelta, "RMSprop": RMSprop,
              "Adagrad": Adagrad, "Adamax": Adamax, "Nadam": Nadam}


def get(opt):
    if isinstance(opt, Optimizer):
        return opt
    if isinstance(opt, str):
        key = {k.lower(): k for k in OPTIMIZERS}.get(opt.lower())
        if key is None:
            raise ValueError(f"unknown optimizer {opt!r}")
        return OPTIMIZERS[key]()
    raise TypeError(f"not a Keras optimizer: {opt!r}")


def serialize(opt: Optimizer) -> dict:
    return {"class_name": type(opt).__name__, "config": opt.get_config()}


def deserialize(cfg: dict, custom_objects=None):
    custom_objects = custom_objects or {}
    name = cfg["class_name"]
    cls = custom_objects.get(name) or OPTIMIZERS.get(name)
    if cls is None:
        raise ValueError(f"unknown optimizer class {name!r}")
    return cls.from_config(cfg["config"])
