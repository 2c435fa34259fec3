"""Device-resident L-BFGS: `LBFGS`, a torch.optim.LBFGS with the same
constructor whose step() keeps the whole iteration on the GPU.

The reference trains the Reddit classifier with optim.LBFGS(lr=1) for two
steps (reddit.py:51-64).  torch's step() synchronises with the host on every
dot product of the two-loop recursion and on every termination test, which at
SGC's sizes (a 24,723-float parameter vector) costs more than the closures.
Here step() evaluates the closure, then enqueues one launch
(sgc_lbfgs_iterate_f32, include/sgc_amd.h) that runs torch's termination
tests, memory update, two-loop recursion, step size and parameter update on
the device, and reads the status back once at the end of the step.  Closures
enqueued after the device has stopped are wasted work, not errors: the launch
is then a no-op and the parameters no longer move (`poll_every=k` reads the
stop word every k iterations and leaves the loop early; same results).

The device path is taken when every parameter is a contiguous real fp32
tensor on one ROCm device, there are at most 16 of them with at most 65,536
elements in all, history_size <= 1024 and line_search_fn is None.  Anything
else -- CPU tensors (the reference's --no-cuda mode), strong-Wolfe, larger
models -- is torch.optim.LBFGS.step itself, bit for bit.

LBFGS.run_steps(model, features, labels, steps) is `steps` such steps with the
reference closure (zero_grad, F.cross_entropy(model(features), labels),
backward).  It is one host call (sgc_train_lbfgs_f32: the closures too are
launches behind the device stop word, so a stopped step costs empty launches
only) and one read-back of the per-step status table when: the device path
above holds; the model is exactly sgc_amd.models.SGC with a bias and the
optimiser's parameters are [W.weight, W.bias] in that order; the features are
float32 on the parameters' ROCm device, 2-D with K columns (copied only where
the layout needs it), or bfloat16 / float16 there in a layout
sgc_linear_xent_x16_kernel_name covers as it lies in memory (even pitch, 4-B
aligned base, at most 48 classes: sgc_train_lbfgs_x16, X read at 16 bits); the
labels are int64 on that device, one per row, none of them -100; and there are
at most 64 classes.  Anything else -- CPU tensors, 16-bit features at an odd
pitch (no re-pitching copy is made here, unlike Adam.run_epochs: the literal
loop is the pinned behaviour for them), rows labelled -100, strong-Wolfe, more
than 64 classes, a foreign model, another parameter order -- is the literal
loop of step() calls.  The fused run is bit-identical to the stepwise device
path driven with the closure `sgc_cross_entropy(model, x, y).backward()`
(float32 features) or with `propagate.linear_xent(x, W, b, y)` assigning
.grad (16-bit features).

LBFGS(..., wide=True) lifts the 65,536-element limit: above it step() drives
sgc_lbfgs_wide_iterate_f32, the same iteration in Gram form spread over the
machine (csrc/lbfgs_wide.hip, six launches per iteration whatever the sizes);
at or below it the narrow kernel runs as before, bit for bit.  run_steps then
also takes TextSGC's training (sgc_amd.textsgc: a model without a bias, the
L2 term `l2`); see the method.  The default, wide=False, is the class as it
was.

Results of the device path are tolerance-equal to torch's (fp64-accumulated
dot products in a fixed order; torch sums in fp32) and bitwise reproducible
run to run.  state_dict() does not carry the device state.

`Adam` is torch.optim.Adam (the citation loop's optimiser, citation.py:41-50)
with torch's constructor and torch's state layout -- state[p] = {"step",
"exp_avg", "exp_avg_sq"}, so state_dict() / load_state_dict() round-trip and
the device path and torch's own step() can alternate on one optimiser.
step() is one sgc_adam_step_f32 launch per param group; run_epochs() is the
whole training loop in one host call (sgc_train_adam_f32).  See the class.
"""
import collections
import ctypes
import weakref

import torch
import torch.nn.functional as F

from . import _lib
from .propagate import X16_DTYPES, is_x16, xent_x16_layout

MAX_NUMEL = 65536
WIDE_MAX_NUMEL = 2 ** 31 - 1  # LBFGS(wide=True): sgc_lbfgs_wide_iterate_f32's limit
_SGC_ERANGE = 2  # include/sgc_amd.h
MAX_TENSORS = 16
MAX_HISTORY = 1024

STOP_NONE, STOP_OPT_AT_ENTRY, STOP_MAX_ITER, STOP_MAX_EVAL, STOP_OPT, STOP_GTD, \
    STOP_STEP_SMALL, STOP_LOSS_CHANGE = range(8)


# The calls of one engine (narrow: csrc/lbfgs.hip, wide: csrc/lbfgs_wide.hip),
# chosen once per optimiser, when its device state is built.
_Engine = collections.namedtuple("_Engine", "workspace init begin_step iterate read_status wide")


def _engine(lib, wide):
    w = "wide_" if wide else ""
    return _Engine(*[getattr(lib, f"sgc_lbfgs_{w}{name}") for name in
                     ("workspace", "init", "begin_step", "iterate_f32", "read_status")], bool(wide))


def _read_status(engine, state, stream):
    """(n_iter, func_evals, iters, evals, stop, hist_len): the one host
    synchronisation of a step."""
    out = (ctypes.c_int64 * 6)()
    _lib.check(engine.read_status(_lib.ptr(state), out, stream), "lbfgs_read_status")
    return tuple(out)


def _grow_ws(owner, nbytes, dev):
    """owner._train_ws, the workspace of the owner's fused calls: kept between
    calls, replaced when too small or on another device."""
    ws = getattr(owner, "_train_ws", None)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = owner._train_ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    return ws


def _read_status_trace(table):
    """run_steps' status table as one tuple per step: the one read-back (and
    host synchronisation) of a fused run."""
    return [tuple(row) for row in table.cpu().view(-1, 6).tolist()]


class _WideOption(type(torch.optim.LBFGS)):
    """LBFGS(..., wide=False): the keyword is taken off before __init__, whose
    signature stays torch's plus poll_every."""

    def __call__(cls, *args, wide=False, **kwargs):
        opt = super().__call__(*args, **kwargs)
        opt.wide = bool(wide)
        return opt


class LBFGS(torch.optim.LBFGS, metaclass=_WideOption):
    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                 tolerance_change=1e-9, history_size=100, line_search_fn=None, poll_every=None):
        super().__init__(params, lr=lr, max_iter=max_iter, max_eval=max_eval,
                         tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                         history_size=history_size, line_search_fn=line_search_fn)
        if poll_every is not None and int(poll_every) < 1:
            raise ValueError(f"poll_every must be None or >= 1, got {poll_every}")
        self.poll_every = None if poll_every is None else int(poll_every)
        self.wide = False       # LBFGS(..., wide=True): see the module docstring
        self._dev_wide = False  # the device state is sgc_lbfgs_wide_workspace's
        self._engine = None     # the _Engine that built the device state
        self._dev_state = None  # uint8 device tensor (sgc_lbfgs_workspace bytes)
        self._dev_key = None    # (parameter identities and shapes, history_size) it was built for
        self.last_status = None  # (n_iter, func_evals, iters, evals, stop, hist_len) of the last step
        self.step_statuses = []  # the same per step of the last run_steps()

    def device_path(self):
        """Whether step() runs on the device (see the module docstring)."""
        group = self.param_groups[0]
        ps = self._params
        if group["line_search_fn"] is not None or not 1 <= len(ps) <= MAX_TENSORS:
            return False
        if not 1 <= group["history_size"] <= MAX_HISTORY or group["max_iter"] < 1:
            return False
        dev = ps[0].device
        if dev.type != "cuda":
            return False
        for p in ps:
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                return False
        n = sum(p.numel() for p in ps)
        return 1 <= n <= MAX_NUMEL or (self.wide and MAX_NUMEL < n < WIDE_MAX_NUMEL)

    def _key(self):
        return (tuple((id(p), p.numel()) for p in self._params),
                self.param_groups[0]["history_size"])

    @torch.no_grad()
    def step(self, closure):
        if self._dev_state is None and not self.device_path():
            return super().step(closure)
        if self._dev_state is not None and (self._key() != self._dev_key or not self.device_path()):
            raise ValueError("sgc_amd.optim.LBFGS: the parameter list or history_size changed "
                             "after the first step")
        lib = _lib.load()
        group = self.param_groups[0]
        ps = self._params
        dev = ps[0].device
        closure = torch.enable_grad()(closure)
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            wide = self._dev_wide if self._dev_state is not None else \
                sum(p.numel() for p in ps) > MAX_NUMEL
            state = self._ensure_state(lib, dev, stream, wide)
            eng = self._engine
            nt = len(ps)
            p_ptrs = (ctypes.c_void_p * nt)(*[p.data_ptr() for p in ps])
            numels = (ctypes.c_int64 * nt)(*[p.numel() for p in ps])
            lr = float(group["lr"])
            _lib.check(eng.begin_step(_lib.ptr(state), stream), "lbfgs_begin_step")
            orig_loss = None
            status = None
            for it in range(group["max_iter"]):
                loss = closure()
                if orig_loss is None:
                    orig_loss = loss
                dloss = self._device_loss(loss, dev)
                grads = [self._dense_grad(p) for p in ps]  # kept alive until the launch is queued
                g_ptrs = (ctypes.c_void_p * nt)(*[None if g is None else g.data_ptr()
                                                  for g in grads])
                _lib.check(eng.iterate(
                    _lib.ptr(state), nt, p_ptrs, g_ptrs, numels, _lib.ptr(dloss), lr,
                    group["max_iter"], group["max_eval"], float(group["tolerance_grad"]),
                    float(group["tolerance_change"]), stream), "lbfgs_iterate_f32")
                if self.poll_every and (it + 1) % self.poll_every == 0 and \
                        it + 1 < group["max_iter"]:
                    status = _read_status(eng, state, stream)
                    if status[4] != STOP_NONE:
                        break
                    status = None
            if status is None:
                status = _read_status(eng, state, stream)
        self.last_status = status
        st = self.state[ps[0]]
        st["n_iter"], st["func_evals"] = int(status[0]), int(status[1])
        return orig_loss

    def _ensure_state(self, lib, dev, stream, wide=False):
        """The device state, built (and zeroed) on first use: the narrow
        kernel's, or with `wide` sgc_lbfgs_wide_workspace's."""
        if self._dev_state is None:
            group = self.param_groups[0]
            n = sum(p.numel() for p in self._params)
            eng = _engine(lib, wide)
            nbytes = eng.workspace(n, group["history_size"])
            if nbytes <= 0:
                _lib.check(1, "lbfgs_workspace")
            state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(eng.init(_lib.ptr(state), nbytes, n, group["history_size"], stream),
                       "lbfgs_init")
            self._dev_state, self._dev_key, self._dev_wide = state, self._key(), eng.wide
            self._engine = eng
        elif self._dev_wide != bool(wide):
            raise ValueError("sgc_amd.optim.LBFGS: the device state was built by the %s kernel; "
                             "one optimiser cannot alternate between the two" %
                             ("wide" if self._dev_wide else "narrow"))
        return self._dev_state

    # -- whole steps in one host call ---------------------------------------------------
    def _fused_plan(self, model, features, labels, wide=False):
        """(W, b, x) when run_steps can run as one sgc_train_lbfgs_f32 /
        sgc_train_lbfgs_x16 call on x (the features in the layout the call
        takes).  With `wide` (and wide=True at construction) the plan of one
        sgc_train_lbfgs_wide_f32 call instead: the model may also be an
        sgc_amd.textsgc.SGC, the bias may be missing (b is None) and the
        features are float32."""
        from .models import SGC
        kinds = (SGC,)
        if wide:
            from .textsgc import SGC as TextSGC
            kinds = (SGC, TextSGC)
        if (wide and not self.wide) or type(model) not in kinds or not self.device_path():
            return None
        W, b = model.W.weight, model.W.bias
        if b is None and not wide:
            return None
        ps = self._params
        if len(ps) != (1 if b is None else 2) or ps[0] is not W or (b is not None and
                                                                    ps[1] is not b):
            return None
        x, y = features, labels
        if not (isinstance(x, torch.Tensor) and x.device == W.device and
                (x.dtype == torch.float32 or (is_x16(x) and not wide)) and x.dim() == 2 and
                x.shape[0] >= 1 and x.shape[1] == W.shape[1] and 1 <= W.shape[0] <= 64):
            return None
        if not (isinstance(y, torch.Tensor) and y.dtype == torch.int64 and y.device == x.device and
                y.shape == (x.shape[0],)):
            return None
        if not (W.requires_grad and (b is None or b.requires_grad)):
            return None
        x = x.detach()
        if is_x16(x):
            # 16-bit features: only as they lie in memory (no re-pitching copy)
            x = xent_x16_layout(x, W.shape[0], copy=False)
            if x is None:
                return None
        elif x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.contiguous()
        if _labels_have_ignored(y, W.shape[0]):
            return None
        return W, b, x

    def _run_fused(self, plan, labels, steps, l2, wide):
        """run_steps' fused path: one sgc_train_lbfgs_f32 / _x16 call, or with
        `wide` one sgc_train_lbfgs_wide_f32 call (the only one that takes l2),
        and one read-back of the status table.  None (no device state built,
        no launch) when the wide call's shape is past the fused closure's
        31-bit offset limits, which it reports as SGC_ERANGE from its argument
        checks: the literal loop runs then."""
        if self._dev_state is not None and self._key() != self._dev_key:
            raise ValueError("sgc_amd.optim.LBFGS: the parameter list or history_size changed "
                             "after the first step")
        W, b, x = plan
        self.zero_grad(set_to_none=True)
        group = self.param_groups[0]
        y = labels.contiguous()
        M, K = x.shape
        C = W.shape[0]
        dev = x.device
        lib = _lib.load()
        kind = "wide_f32" if wide else "x16" if is_x16(x) else "f32"
        train = getattr(lib, "sgc_train_lbfgs_" + kind)
        ws_bytes = getattr(lib, {"wide_f32": "sgc_train_lbfgs_wide_workspace",
                                 "x16": "sgc_train_lbfgs_x16_workspace",
                                 "f32": "sgc_train_lbfgs_workspace"}[kind])(M, K, C)
        ws = _grow_ws(self, ws_bytes, dev)
        losses = torch.empty(steps, dtype=torch.float32, device=dev)
        table = torch.empty(steps * 6, dtype=torch.int64, device=dev)
        head = (_lib.ptr(x), X16_DTYPES[x.dtype], x.stride(0)) if kind == "x16" else \
            (_lib.ptr(x), x.stride(0))
        tols = (float(group["tolerance_grad"]), float(group["tolerance_change"])) + \
            ((l2,) if wide else ())
        with torch.no_grad(), torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)

            def call(state, n_steps):
                return train(*head, _lib.ptr(W), None if b is None else _lib.ptr(b), _lib.ptr(y),
                             M, K, C, _lib.ptr(state), n_steps, float(group["lr"]),
                             group["max_iter"], group["max_eval"], *tols, _lib.ptr(losses),
                             _lib.ptr(table), _lib.ptr(ws), ws.numel(), stream)
            # the argument checks alone (steps = 0 returns after them, before
            # the state is looked at): a shape the closure refuses has no plan
            if wide and (ws_bytes <= 0 or call(ws, 0) == _SGC_ERANGE):
                return None
            _lib.check(call(self._ensure_state(lib, dev, stream, wide), steps),
                       "train_lbfgs_" + kind)
            self.step_statuses = _read_status_trace(table)
        self.last_status = self.step_statuses[-1]
        st = self.state[self._params[0]]
        st["n_iter"], st["func_evals"] = int(self.last_status[0]), int(self.last_status[1])
        return losses

    def run_steps(self, model, features, labels, steps, l2=0.0):
        """`steps` times self.step(closure) with the reference closure --
        zero_grad, F.cross_entropy(model(features), labels), backward
        (reddit.py:51-64).  Returns the [steps] tensor of each step's first
        closure loss (what step() returns), None when steps == 0 (nothing is
        touched).  Afterwards `step_statuses` holds one status tuple per step
        (None for a step torch's own step() ran) and `last_status` the last.

        The fused path (module docstring) is one sgc_train_lbfgs_f32 call
        (sgc_train_lbfgs_x16 on bfloat16 / float16 features that are covered
        as they lie in memory -- even pitch, 4-B aligned; an odd pitch runs
        the literal loop, where Adam.run_epochs would copy once) and
        one read-back of the status table, the call's only synchronisation
        after the labels' one range check; the parameters' .grad is left None.
        Everything else runs the literal loop.  A label outside [0, C) other
        than -100 raises IndexError on either path.

        `l2` adds TextSGC's term 0.5 * l2 * (model.W.weight ** 2).sum() to the
        closure (reference downstream/TextSGC/train.py:65-71; never on the
        bias).  With wide=True the fused path also covers a model without a
        bias, sgc_amd.textsgc.SGC, any parameter count and l2 != 0, all as one
        sgc_train_lbfgs_wide_f32 call on float32 features; a model the narrow
        call covers keeps the narrow call (and its bits) while l2 == 0.
        A shape past the fused closure's 31-bit offset limits (the call's
        SGC_ERANGE) and, without wide=True, l2 != 0 run the literal loop."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"steps must be >= 0, got {steps}")
        if steps == 0:
            return None
        l2 = float(l2)
        plan = None
        if l2 == 0.0 and not (self._dev_state is not None and self._dev_wide) and \
                sum(p.numel() for p in self._params) <= MAX_NUMEL:
            plan = self._fused_plan(model, features, labels)
        if plan is None and not (self._dev_state is not None and not self._dev_wide):
            wide_plan = self._fused_plan(model, features, labels, wide=True)
            if wide_plan is not None:
                model.train()
                losses = self._run_fused(wide_plan, labels, steps, l2, True)
                if losses is not None:
                    return losses
        model.train()
        if plan is None:
            def closure():
                self.zero_grad()
                loss = F.cross_entropy(model(features), labels)
                if l2 != 0.0:
                    loss = loss + 0.5 * l2 * (model.W.weight ** 2).sum()
                loss.backward()
                return loss
            losses, self.step_statuses = [], []
            for _ in range(steps):
                self.last_status = None
                loss = self.step(closure)
                losses.append(torch.as_tensor(loss).detach())
                self.step_statuses.append(self.last_status)
            return torch.stack(losses)
        return self._run_fused(plan, labels, steps, l2, False)

    @staticmethod
    def _device_loss(loss, dev):
        """The closure's value as one fp32 scalar on `dev` (a Python float or
        a CPU tensor is copied there)."""
        if isinstance(loss, torch.Tensor) and loss.device == dev:
            x = loss.detach().reshape(-1)
            if x.numel() != 1:
                raise ValueError("sgc_amd.optim.LBFGS: the closure must return a scalar loss")
            return x if x.dtype == torch.float32 else x.to(torch.float32)
        return torch.tensor([float(loss)], dtype=torch.float32).to(dev)

    @staticmethod
    def _dense_grad(p):
        g = p.grad
        if g is None:
            return None
        if g.is_sparse:
            g = g.to_dense()
        if g.dtype != torch.float32 or g.device != p.device:
            g = g.to(device=p.device, dtype=torch.float32)
        return g.contiguous()


_label_checks = {}  # id(labels) -> (weak reference, (version, C), has ignored rows)


def _forget_label_check(ref, key):
    hit = _label_checks.get(key)
    if hit is not None and hit[0] is ref:
        del _label_checks[key]


def _labels_have_ignored(labels, C):
    """Range check of run_epochs' labels, once (one host synchronisation) per
    labels tensor object and version, as models._check_labels keeps its
    passes: a label outside [0, C) other than -100 raises IndexError as torch
    does; -> whether any row carries ignore_index (-100), which the fused
    loop does not compute."""
    key = id(labels)
    state = (labels._version, int(C))
    hit = _label_checks.get(key)
    if hit is not None and hit[0]() is labels and hit[1] == state:
        return hit[2]
    outside = (labels < 0) | (labels >= C)
    ignored = False
    if bool(outside.any()):
        bad = outside & (labels != -100)
        if bool(bad.any()):
            y = int(labels[bad][0])
            raise IndexError(f"Target {y} is out of bounds (classes: {C}, ignore_index: -100)")
        ignored = True
    if len(_label_checks) > 64:
        _label_checks.clear()
    _label_checks[key] = (weakref.ref(labels, lambda r, key=key: _forget_label_check(r, key)),
                          state, ignored)
    return ignored


def _is_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


class Adam(torch.optim.Adam):
    """torch.optim.Adam whose step() and whole training loop run on the HIP
    kernels (sgc_adam_step_f32, sgc_train_adam_f32; the arithmetic and its
    operation order: include/sgc_amd.h).

    step(closure=None) takes the device path -- one launch per param group,
    state["step"] advanced on the host as torch's non-capturable path does --
    when, in every group, each parameter with a gradient is a contiguous
    float32 tensor on one ROCm device with a dense float32 gradient, there are
    at most 16 of them, amsgrad / maximize / capturable / differentiable /
    fused / decoupled_weight_decay are off, and lr and the betas are Python
    numbers.  Anything else is torch.optim.Adam.step itself, bit for bit (CPU
    tensors: the reference's --no-cuda mode).

    run_epochs(model, features, labels, epochs) is the loop of
    citation.py:44-50 in one host call; see the method.

    Device results are tolerance-equal to torch's (not bit-equal) and bitwise
    reproducible run to run.
    """

    # -- step -----------------------------------------------------------------------
    @staticmethod
    def _group_plain(group):
        return not (group["amsgrad"] or group["maximize"] or group["capturable"] or
                    group["differentiable"] or group["fused"] or
                    group.get("decoupled_weight_decay", False)) and \
            _is_number(group["lr"]) and all(_is_number(b) for b in group["betas"]) and \
            _is_number(group["eps"]) and _is_number(group["weight_decay"])

    def _device_group(self, group):
        """The group's parameters with a gradient when the group can take the
        device path, else None."""
        if not self._group_plain(group):
            return None
        ps = [p for p in group["params"] if p.grad is not None]
        if len(ps) > MAX_TENSORS:
            return None
        dev = None
        for p in ps:
            g = p.grad
            if (p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous() or
                    g.is_sparse or g.layout != torch.strided or g.dtype != torch.float32 or
                    g.device != p.device or not g.is_contiguous() or
                    (dev is not None and p.device != dev)):
                return None
            dev = p.device
            st = self.state.get(p)
            if st:
                if (st["step"].device.type != "cpu" or not st["exp_avg"].is_contiguous() or
                        not st["exp_avg_sq"].is_contiguous() or
                        st["exp_avg"].dtype != torch.float32 or
                        st["exp_avg_sq"].dtype != torch.float32):
                    return None
        return ps

    def _init_state(self, p):
        """torch's lazy state initialisation (Adam._init_group, the
        non-capturable, non-fused form: the step count lives on the host)."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() ==
                                      torch.float64 else torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        plans = [self._device_group(g) for g in self.param_groups]
        if any(ps is None for ps in plans):
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
            plans = [self._device_group(g) for g in self.param_groups]  # the closure's gradients
            if any(ps is None for ps in plans):
                # (the closure has run: torch's step takes its gradients as they are)
                super().step(None)
                return loss
        if not any(plans):  # no parameter has a gradient: nothing moves (as torch)
            return loss
        lib = _lib.load()
        for group, ps in zip(self.param_groups, plans):
            if not ps:
                continue
            states = [self._init_state(p) for p in ps]
            dev = ps[0].device
            nt = len(ps)
            b1, b2 = group["betas"]
            # one launch per run of parameters that share a step count (as a
            # rule all of them: one launch)
            steps = [int(st["step"].tolist()) + 1 for st in states]
            for step in sorted(set(steps)):
                idx = [i for i in range(nt) if steps[i] == step]
                n = len(idx)
                arr = lambda xs: (ctypes.c_void_p * n)(*xs)  # noqa: E731
                with torch.cuda.device(dev):
                    _lib.check(lib.sgc_adam_step_f32(
                        n, arr([ps[i].data_ptr() for i in idx]),
                        arr([ps[i].grad.data_ptr() for i in idx]),
                        arr([states[i]["exp_avg"].data_ptr() for i in idx]),
                        arr([states[i]["exp_avg_sq"].data_ptr() for i in idx]),
                        (ctypes.c_int64 * n)(*[ps[i].numel() for i in idx]), step,
                        float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                        float(group["weight_decay"]), _lib.stream_handle(dev)), "adam_step_f32")
            for st in states:
                st["step"] += 1
        return loss

    # -- the whole loop ---------------------------------------------------------------
    def _fused_plan(self, model, features, labels):
        """(W, b, x) when run_epochs can run as one sgc_train_adam_f32 /
        sgc_train_adam_x16 call on x (the features in the layout the call
        takes: 16-bit features after at most one even-pitch copy)."""
        from .models import SGC
        if type(model) is not SGC or model.W.bias is None or len(self.param_groups) != 1:
            return None
        group = self.param_groups[0]
        W, b = model.W.weight, model.W.bias
        ps = group["params"]
        if len(ps) != 2 or not ((ps[0] is W and ps[1] is b) or (ps[0] is b and ps[1] is W)):
            return None
        if not self._group_plain(group):
            return None
        x, y = features, labels
        if not (isinstance(x, torch.Tensor) and x.device.type == "cuda" and
                (x.dtype == torch.float32 or is_x16(x)) and x.dim() == 2 and x.shape[0] >= 1 and
                x.shape[1] == W.shape[1] and 1 <= W.shape[0] <= 64):
            return None
        if not (isinstance(y, torch.Tensor) and y.dtype == torch.int64 and y.device == x.device and
                y.shape == (x.shape[0],)):
            return None
        for p in (W, b):
            if (p.device != x.device or p.dtype != torch.float32 or not p.is_contiguous() or
                    not p.requires_grad):
                return None
            st = self.state.get(p)
            if st and (st["step"].device.type != "cpu" or not st["exp_avg"].is_contiguous() or
                       not st["exp_avg_sq"].is_contiguous() or
                       st["exp_avg"].dtype != torch.float32 or
                       st["exp_avg_sq"].dtype != torch.float32):
                return None
        sw, sb = self.state.get(W), self.state.get(b)
        if bool(sw) != bool(sb) or (sw and sw["step"].tolist() != sb["step"].tolist()):
            return None
        if _labels_have_ignored(y, W.shape[0]):
            return None
        x = x.detach()
        if is_x16(x):
            x = xent_x16_layout(x, W.shape[0])  # one even-pitch copy per call where needed
            if x is None:
                return None
        elif x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.contiguous()
        return W, b, x

    def run_epochs(self, model, features, labels, epochs, loss_trace=False):
        """The training loop of citation.py:44-50 -- `epochs` times zero_grad,
        F.cross_entropy(model(features), labels), backward, step -- on an
        sgc_amd.models.SGC model whose two parameters form this optimiser's
        one param group.  On ROCm float32 features with at most 64 classes it
        is one call of sgc_train_adam_f32, on bfloat16 / float16 features that
        sgc_linear_xent_x16_kernel_name covers (at most 48 classes) one call
        of sgc_train_adam_x16 after at most one even-pitch copy per call
        (Cora's 1433 and Citeseer's 3703 are odd; LBFGS.run_steps makes no
        such copy and runs its literal loop instead): no launch is issued from Python per
        epoch and, after the labels' one range check (once per labels tensor
        object and version), nothing synchronises with the host.

        Returns the last epoch's loss (the mean cross-entropy at the weights
        before that epoch's update, what the reference's loop computes last)
        as a 0-d tensor, or the [epochs] trace with loss_trace=True; None when
        epochs == 0 (nothing is touched).

        Afterwards the weights, exp_avg, exp_avg_sq and step (advanced by
        `epochs`) are the state `epochs` calls of step() would have left, so a
        later step() or run_epochs() continues from there.  The fused loop
        forms no gradient tensors: the parameters' .grad is left None.

        Everything else -- CPU tensors, uncovered 16-bit features, more than 64 classes,
        a bias-free or foreign model, a param group step() would hand to
        torch, rows labelled -100 -- runs the literal Python loop with
        self.step() (on the CPU bit-equal to torch.optim.Adam driving the same
        loop).  A label outside [0, C) other than -100 raises IndexError."""
        epochs = int(epochs)
        if epochs < 0:
            raise ValueError(f"epochs must be >= 0, got {epochs}")
        if epochs == 0:
            return None
        plan = self._fused_plan(model, features, labels)
        if plan is None:
            losses = []
            for _ in range(epochs):
                model.train()
                self.zero_grad()
                loss = F.cross_entropy(model(features), labels)
                loss.backward()
                self.step()
                losses.append(loss.detach())
            return torch.stack(losses) if loss_trace else losses[-1]
        W, b, x = plan
        model.train()
        self.zero_grad(set_to_none=True)
        group = self.param_groups[0]
        y = labels.contiguous()
        M, K = x.shape
        C = W.shape[0]
        dev = x.device
        sw, sb = self._init_state(W), self._init_state(b)
        step0 = int(sw["step"].tolist())
        lib = _lib.load()
        x16 = is_x16(x)
        ws_bytes = (lib.sgc_train_adam_x16_workspace if x16 else
                    lib.sgc_train_adam_workspace)(M, K, C)
        ws = _grow_ws(self, ws_bytes, dev)
        trace = torch.empty(epochs, dtype=torch.float32, device=dev)
        b1, b2 = group["betas"]
        with torch.no_grad(), torch.cuda.device(dev):
            tail = (_lib.ptr(W), _lib.ptr(b), _lib.ptr(y), M, K, C, _lib.ptr(sw["exp_avg"]),
                    _lib.ptr(sw["exp_avg_sq"]), _lib.ptr(sb["exp_avg"]), _lib.ptr(sb["exp_avg_sq"]),
                    step0, epochs, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                    float(group["weight_decay"]), _lib.ptr(trace), _lib.ptr(ws), ws.numel(),
                    _lib.stream_handle(dev))
            if x16:
                _lib.check(lib.sgc_train_adam_x16(_lib.ptr(x), X16_DTYPES[x.dtype], x.stride(0),
                                                  *tail), "train_adam_x16")
            else:
                _lib.check(lib.sgc_train_adam_f32(_lib.ptr(x), x.stride(0), *tail),
                           "train_adam_f32")
        for st in (sw, sb):
            st["step"] += epochs
        return trace if loss_trace else trace[-1]
