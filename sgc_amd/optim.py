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

Results of the device path are tolerance-equal to torch's (fp64-accumulated
dot products in a fixed order; torch sums in fp32) and bitwise reproducible
run to run.  state_dict() does not carry the device state.
"""
import ctypes

import torch

from . import _lib

MAX_NUMEL = 65536
MAX_TENSORS = 16
MAX_HISTORY = 1024

STOP_NONE, STOP_OPT_AT_ENTRY, STOP_MAX_ITER, STOP_MAX_EVAL, STOP_OPT, STOP_GTD, \
    STOP_STEP_SMALL, STOP_LOSS_CHANGE = range(8)


def _read_status(lib, state, stream):
    """(n_iter, func_evals, iters, evals, stop, hist_len): the one host
    synchronisation of a step."""
    out = (ctypes.c_int64 * 6)()
    _lib.check(lib.sgc_lbfgs_read_status(_lib.ptr(state), out, stream), "lbfgs_read_status")
    return tuple(out)


class LBFGS(torch.optim.LBFGS):
    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                 tolerance_change=1e-9, history_size=100, line_search_fn=None, poll_every=None):
        super().__init__(params, lr=lr, max_iter=max_iter, max_eval=max_eval,
                         tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                         history_size=history_size, line_search_fn=line_search_fn)
        if poll_every is not None and int(poll_every) < 1:
            raise ValueError(f"poll_every must be None or >= 1, got {poll_every}")
        self.poll_every = None if poll_every is None else int(poll_every)
        self._dev_state = None  # uint8 device tensor (sgc_lbfgs_workspace bytes)
        self._dev_key = None    # (parameter identities and shapes, history_size) it was built for
        self.last_status = None  # (n_iter, func_evals, iters, evals, stop, hist_len) of the last step

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
        return 1 <= sum(p.numel() for p in ps) <= MAX_NUMEL

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
        n = sum(p.numel() for p in ps)
        closure = torch.enable_grad()(closure)
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            if self._dev_state is None:
                nbytes = lib.sgc_lbfgs_workspace(n, group["history_size"])
                if nbytes <= 0:
                    _lib.check(1, "lbfgs_workspace")
                state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _lib.check(lib.sgc_lbfgs_init(_lib.ptr(state), nbytes, n, group["history_size"],
                                              stream), "lbfgs_init")
                self._dev_state, self._dev_key = state, self._key()
            state = self._dev_state
            nt = len(ps)
            p_ptrs = (ctypes.c_void_p * nt)(*[p.data_ptr() for p in ps])
            numels = (ctypes.c_int64 * nt)(*[p.numel() for p in ps])
            lr = float(group["lr"])
            _lib.check(lib.sgc_lbfgs_begin_step(_lib.ptr(state), stream), "lbfgs_begin_step")
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
                _lib.check(lib.sgc_lbfgs_iterate_f32(
                    _lib.ptr(state), nt, p_ptrs, g_ptrs, numels, _lib.ptr(dloss), lr,
                    group["max_iter"], group["max_eval"], float(group["tolerance_grad"]),
                    float(group["tolerance_change"]), stream), "lbfgs_iterate_f32")
                if self.poll_every and (it + 1) % self.poll_every == 0 and \
                        it + 1 < group["max_iter"]:
                    status = _read_status(lib, state, stream)
                    if status[4] != STOP_NONE:
                        break
                    status = None
            if status is None:
                status = _read_status(lib, state, stream)
        self.last_status = status
        st = self.state[ps[0]]
        st["n_iter"], st["func_evals"] = int(status[0]), int(status[1])
        return orig_loss

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
