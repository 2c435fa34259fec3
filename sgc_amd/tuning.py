"""The weight-decay search of the reference's tuning.py as one batch:
`ModelBank`, `AdamSweep` and `sample_weight_decays`.

The reference trains 60 independent SGC classifiers in sequence, each for 100
epochs on the same features[idx_train] (tuning.py:26-33); the trials differ in
their initial weights and in one scalar, the weight decay.  Here the trials
are the batch dimension of the fused Adam loop: a ModelBank stacks B models'
parameters, AdamSweep.run_epochs trains all of them in one host call
(sgc_train_adam_sweep_f32: the small schedule's two launches per epoch on a
K-block x model grid) and ModelBank.evaluate takes every model's validation
counts in one more (sgc_linear_eval_sweep_f32).  Model i's results are
bit-identical to its own sgc_amd.optim.Adam.run_epochs / SGC.evaluate.

The search itself is a random search -- log-uniform draws over the
reference's space (tuning.py:21), all evaluated at once -- not hyperopt's TPE:
TPE proposes trial t + 1 from the results of trials 1..t, the sequential loop
the batch replaces.  drivers/tuning.py is the command-line counterpart.
"""
import math

import numpy as np
import torch

from . import _lib
from .metrics import Evaluation
from .models import SGC, _check_eval_labels
from .optim import Adam, _grow_ws, _labels_have_ignored

MAX_MODELS = 4096


def sample_weight_decays(n, low=1e-10, high=1e-4, seed=0):
    """n log-uniform draws from [low, high] -- the reference's search space
    hp.loguniform(log(1e-10), log(1e-4)) (tuning.py:21) -- as a float64 numpy
    array, from numpy.random.RandomState(seed): the same draws for the same
    seed."""
    n = int(n)
    if n < 0 or not 0 < low <= high:
        raise ValueError("sample_weight_decays: n >= 0 and 0 < low <= high expected")
    rs = np.random.RandomState(seed)
    return np.exp(rs.uniform(math.log(low), math.log(high), n))


class ModelBank:
    """B sgc_amd.models.SGC models of one shape on one device, their
    parameters stacked: `.weight` [B, C, K] and `.bias` [B, C].  Each model's
    W.weight.data / W.bias.data is rebound to its slice of the stacks, so every
    model stays usable on its own -- model(x), model.evaluate, Adam.run_epochs
    -- and sees what a sweep wrote.  (Moving a model afterwards -- .cuda(),
    .to() -- rebinds its parameters away from the bank; the bank then runs
    model by model.)"""

    def __init__(self, models):
        models = list(models)
        if not 1 <= len(models) <= MAX_MODELS:
            raise ValueError(f"ModelBank: 1..{MAX_MODELS} models expected, got {len(models)}")
        first = models[0]
        for m in models:
            if type(m) is not SGC or m.W.bias is None:
                raise TypeError("ModelBank: sgc_amd.models.SGC models (with a bias) expected")
            if (m.W.weight.shape != first.W.weight.shape or
                    m.W.weight.device != first.W.weight.device or
                    m.W.weight.dtype != torch.float32 or m.W.bias.dtype != torch.float32 or
                    m.W.bias.device != first.W.weight.device):
                raise ValueError("ModelBank: the models must share one shape and one device")
        if len({id(m) for m in models}) != len(models):
            raise ValueError("ModelBank: the same model twice")
        self.models = models
        with torch.no_grad():
            self.weight = torch.stack([m.W.weight.detach() for m in models]).contiguous()
            self.bias = torch.stack([m.W.bias.detach() for m in models]).contiguous()
        for i, m in enumerate(models):
            m.W.weight.data = self.weight[i]
            m.W.bias.data = self.bias[i]

    def __len__(self):
        return len(self.models)

    @property
    def device(self):
        return self.weight.device

    def bound(self):
        """Whether every model's parameters still are the bank's slices."""
        return all(m.W.weight.data_ptr() == self.weight[i].data_ptr() and
                   m.W.bias.data_ptr() == self.bias[i].data_ptr() and
                   m.W.weight.is_contiguous() and m.W.weight.device == self.weight.device
                   for i, m in enumerate(self.models))

    @torch.no_grad()
    def evaluate(self, features, labels):
        """[model.evaluate(features, labels) for model in the bank]: a list of
        metrics.Evaluation.  On ROCm float32 features that sgc_linear_eval_f32
        covers it is one sgc_linear_eval_sweep_f32 call (no host
        synchronisation after the labels' one range check); everything else
        -- CPU tensors, 16-bit features, more than 64 classes -- calls
        model.evaluate per model.  Either way entry i equals model i's own
        evaluate (bit for bit on the kernel path)."""
        x = features
        B = len(self.models)
        C, K = self.weight.shape[1:]
        fused = (isinstance(x, torch.Tensor) and x.device.type == "cuda" and
                 x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and
                 x.shape[1] == K and x.device == self.weight.device and
                 isinstance(labels, torch.Tensor) and labels.shape == (x.shape[0],) and
                 self.bound())
        if fused:
            x = x.detach()
            if x.stride(1) != 1 or x.stride(0) < K:
                x = x.contiguous()
            lib = _lib.load()
            M = x.shape[0]
            fused = lib.sgc_linear_eval_kernel_name(M, K, x.stride(0), C, _lib.ptr(x)) != b"none"
        if not fused:
            return [m.evaluate(features, labels) for m in self.models]
        _check_eval_labels(labels, C)
        dev = x.device
        y = labels.to(device=dev, dtype=torch.int64).contiguous()
        confusion = torch.empty((B, C, C), dtype=torch.int64, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        ws_bytes = lib.sgc_linear_eval_workspace(M, K, C)
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sgc_linear_eval_sweep_f32(
                _lib.ptr(x), x.stride(0), _lib.ptr(self.weight), _lib.ptr(self.bias), _lib.ptr(y),
                B, M, K, C, None, _lib.ptr(confusion), _lib.ptr(counts), _lib.ptr(loss),
                _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev)), "linear_eval_sweep_f32")
        return [Evaluation(confusion[i], counts[i, 0], counts[i, 1], loss[i], len(labels))
                for i in range(B)]


class AdamSweep:
    """One sgc_amd.optim.Adam per model of a ModelBank -- model i with
    weight_decays[i], all with the same lr, betas and eps -- whose moments are
    slices of two stacks like the bank's parameters, so that run_epochs can
    train the whole bank in one host call.  `.optimizers[i]` is model i's
    optimiser: an ordinary Adam that can also be driven on its own."""

    def __init__(self, bank, lr, weight_decays, betas=(0.9, 0.999), eps=1e-8):
        wds = [float(w) for w in np.asarray(weight_decays, dtype=np.float64).reshape(-1)]
        if len(wds) != len(bank):
            raise ValueError(f"AdamSweep: {len(bank)} models but {len(wds)} weight decays")
        self.bank = bank
        self.weight_decays = wds
        self.optimizers = [Adam([m.W.weight, m.W.bias], lr=lr, weight_decay=wd, betas=betas,
                                eps=eps) for m, wd in zip(bank.models, wds)]
        self._moments = None  # (exp_avg_W, exp_avg_sq_W, exp_avg_b, exp_avg_sq_b) stacks
        self._wd_dev = None   # the decays as float32 on the bank's device (the fused call's table)
        if bank.device.type == "cuda":
            self._wd_dev = torch.tensor(wds, dtype=torch.float32).to(bank.device)
        self._train_ws = None

    def _stack_state(self):
        """The four moment stacks, each optimiser's state bound to its slices
        (created on first use, as torch creates an optimiser's state)."""
        if self._moments is None:
            bank = self.bank
            mW, vW = torch.zeros_like(bank.weight), torch.zeros_like(bank.weight)
            mb, vb = torch.zeros_like(bank.bias), torch.zeros_like(bank.bias)
            for i, (m, opt) in enumerate(zip(bank.models, self.optimizers)):
                for p, avg, sq in ((m.W.weight, mW, vW), (m.W.bias, mb, vb)):
                    st = opt.state[p]
                    if len(st) == 0:  # fresh: Adam._init_state's, on the zeroed slices
                        st["step"] = torch.tensor(
                            0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64
                            else torch.float32)
                    else:
                        avg[i].copy_(st["exp_avg"])
                        sq[i].copy_(st["exp_avg_sq"])
                    st["exp_avg"], st["exp_avg_sq"] = avg[i], sq[i]
            self._moments = (mW, vW, mb, vb)
        return self._moments

    def _state_bound(self):
        mW, vW, mb, vb = self._moments
        for i, (m, opt) in enumerate(zip(self.bank.models, self.optimizers)):
            for p, avg, sq in ((m.W.weight, mW, vW), (m.W.bias, mb, vb)):
                st = opt.state.get(p)
                if not st or st["exp_avg"].data_ptr() != avg[i].data_ptr() or \
                        st["exp_avg_sq"].data_ptr() != sq[i].data_ptr() or \
                        st["step"].device.type != "cpu":
                    return False
        return True

    def _fused_plan(self, features, labels):
        """The features in the layout sgc_train_adam_sweep_f32 takes, or None
        when the call does not apply."""
        bank = self.bank
        x, y = features, labels
        C, K = bank.weight.shape[1:]
        if not (isinstance(x, torch.Tensor) and x.device.type == "cuda" and
                x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and
                x.shape[1] == K and 1 <= C <= 64 and x.device == bank.weight.device):
            return None
        if not (isinstance(y, torch.Tensor) and y.dtype == torch.int64 and y.device == x.device and
                y.shape == (x.shape[0],)):
            return None
        if not bank.bound() or not all(m.W.weight.requires_grad and m.W.bias.requires_grad
                                       for m in bank.models):
            return None
        for opt, wd in zip(self.optimizers, self.weight_decays):
            g = opt.param_groups
            if len(g) != 1 or not Adam._group_plain(g[0]) or g[0]["weight_decay"] != wd or \
                    g[0]["lr"] != self.optimizers[0].param_groups[0]["lr"] or \
                    tuple(g[0]["betas"]) != tuple(self.optimizers[0].param_groups[0]["betas"]) or \
                    g[0]["eps"] != self.optimizers[0].param_groups[0]["eps"]:
                return None
        if _labels_have_ignored(y, C):
            return None
        self._stack_state()
        if not self._state_bound():
            return None
        steps = {opt.state[p]["step"].tolist() for m, opt in zip(bank.models, self.optimizers)
                 for p in (m.W.weight, m.W.bias)}
        if len(steps) != 1:
            return None
        x = x.detach()
        if x.stride(1) != 1 or x.stride(0) < K:
            x = x.contiguous()
        return x

    def run_epochs(self, features, labels, epochs, loss_trace=False):
        """Adam.run_epochs(model, features, labels, epochs) for every model of
        the bank.  Returns the [B] tensor of each model's last-epoch loss, or
        the [B, epochs] traces with loss_trace=True; None when epochs == 0.

        On ROCm float32 features (at most 64 classes, int64 labels none of
        which is -100) it is one sgc_train_adam_sweep_f32 call: nothing is
        launched from Python per model or per epoch and, after the labels' one
        range check, nothing synchronises with the host.  The results --
        weights, moments, losses -- are bit-identical to B separate
        Adam.run_epochs calls with the matching "adam_kernel" (2 where the
        small schedule takes the shape, which the sweep uses at every such
        shape under the default setting 0 as well; 1 elsewhere: include/
        sgc_amd.h).  Everything else -- CPU tensors, 16-bit features, rows
        labelled -100, more than 64 classes -- runs Adam.run_epochs model by
        model, with the results of B separate optimisers.  A label outside
        [0, C) other than -100 raises IndexError.  A second call continues
        from the first."""
        epochs = int(epochs)
        if epochs < 0:
            raise ValueError(f"epochs must be >= 0, got {epochs}")
        if epochs == 0:
            return None
        x = self._fused_plan(features, labels)
        bank = self.bank
        if x is None:
            out = [opt.run_epochs(m, features, labels, epochs, loss_trace=loss_trace)
                   for m, opt in zip(bank.models, self.optimizers)]
            return torch.stack(out)
        B = len(bank)
        C, K = bank.weight.shape[1:]
        M = x.shape[0]
        dev = x.device
        y = labels.contiguous()
        mW, vW, mb, vb = self._moments
        group = self.optimizers[0].param_groups[0]
        step0 = int(self.optimizers[0].state[bank.models[0].W.weight]["step"].tolist())
        if self._wd_dev is None or self._wd_dev.device != dev:
            self._wd_dev = torch.tensor(self.weight_decays, dtype=torch.float32).to(dev)
        lib = _lib.load()
        ws_bytes = lib.sgc_train_adam_sweep_workspace(B, M, K, C)
        ws = _grow_ws(self, ws_bytes, dev)
        trace = torch.empty((B, epochs), dtype=torch.float32, device=dev)
        b1, b2 = group["betas"]
        for m, opt in zip(bank.models, self.optimizers):
            m.train()
            opt.zero_grad(set_to_none=True)
        with torch.no_grad(), torch.cuda.device(dev):
            _lib.check(lib.sgc_train_adam_sweep_f32(
                _lib.ptr(x), x.stride(0), _lib.ptr(bank.weight), _lib.ptr(bank.bias), _lib.ptr(y),
                B, M, K, C, _lib.ptr(mW), _lib.ptr(vW), _lib.ptr(mb), _lib.ptr(vb), step0, epochs,
                float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                _lib.ptr(self._wd_dev), _lib.ptr(trace), _lib.ptr(ws), ws.numel(),
                _lib.stream_handle(dev)), "train_adam_sweep_f32")
        for m, opt in zip(bank.models, self.optimizers):
            for p in (m.W.weight, m.W.bias):
                opt.state[p]["step"] += epochs
        return trace if loss_trace else trace[:, -1]
