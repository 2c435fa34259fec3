"""The weight-decay sweep on the GPU: sgc_train_adam_sweep_f32 and
sgc_linear_eval_sweep_f32 against single-model calls (byte for byte, no
tolerance), their error returns, sgc_amd.tuning's ModelBank / AdamSweep
against separately built twins, and drivers/tuning.py with the --tuned-from
link of drivers/citation.py.

Every device buffer a call may write sits between two runs of PAD filled
elements, which must keep their fill."""
import contextlib
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from adam_ref import BETAS, EPS, LR
from test_gpu_adam import problem

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "drivers"))

DEV = "cuda:0"
PAD = 64
FILL = {torch.float32: 7.0, torch.int64: -77, torch.uint8: 0xA5}
EINVAL, ENOMEM = 1, 4


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def knob(lib, value):
    assert lib.sgc_set_tuning(b"adam_kernel", value) == 0
    try:
        yield
    finally:
        lib.sgc_set_tuning(b"adam_kernel", 0)


@contextlib.contextmanager
def form_knob(lib, value):
    """"adam_sweep_form": 1 the fused launch 2, 2 the split one (0: the rule)."""
    assert lib.sgc_set_tuning(b"adam_sweep_form", value) == 0
    try:
        yield
    finally:
        lib.sgc_set_tuning(b"adam_sweep_form", 0)


class Guarded:
    """A contiguous device tensor `.t` with PAD filled elements on both sides."""

    def __init__(self, shape, dtype=torch.float32, src=None):
        n = int(np.prod(shape))
        self.fill = FILL[dtype]
        self.buf = torch.full((n + 2 * PAD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(shape)
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all()) and bool((self.buf[-PAD:] == self.fill).all())


def guarded_x(X, pad):
    """X [M, K] at ldx = K + pad inside a guarded buffer whose pad columns keep
    the fill (pad > 0: on a base that is only 4-B aligned)."""
    M, K = X.shape
    g = Guarded((M * (K + pad) + (1 if pad else 0),))
    flat = g.t[1:] if pad else g.t
    x = flat.view(M, K + pad)[:, :K]
    x.copy_(X)
    assert x.stride(0) == K + pad and (not pad or x.data_ptr() % 8 == 4)
    return g, x


def decays(B):
    """Distinct fp32 decays, 0.0 in the first, a middle and the last model
    (B = 2: the first only, so that one model decays; B = 1: 0.0)."""
    wd = np.float32(5e-4) * np.float32(0.7) ** np.arange(B, dtype=np.float32)
    zero = {0, B // 2, B - 1} if B >= 3 else {0}
    wd[list(zero)] = 0.0
    assert len(set(wd[wd != 0].tolist())) == int((wd != 0).sum())
    return wd.astype(np.float32)


def initial(B, M, K, C, step0, same_weights=False):
    """X, y and B models' W, b, moments (non-zero moments where step0 > 0)."""
    X, W0, b0, y = problem(M, K, C)
    gen = torch.Generator().manual_seed(5 + B + 7 * step0)
    if same_weights:
        W, b = W0.expand(B, C, K).clone(), b0.expand(B, C).clone()
    else:
        W = W0 * (1 + 0.5 * torch.rand(B, C, K, generator=gen))
        b = b0 * (1 + 0.5 * torch.rand(B, C, generator=gen))
    if step0:
        mW, mb = 1e-3 * torch.randn(B, C, K, generator=gen), 1e-3 * torch.randn(B, C, generator=gen)
        vW, vb = 1e-5 * torch.rand(B, C, K, generator=gen), 1e-5 * torch.rand(B, C, generator=gen)
    else:
        mW, vW, mb, vb = (torch.zeros(B, C, K), torch.zeros(B, C, K), torch.zeros(B, C),
                          torch.zeros(B, C))
    return X, y, dict(W=W, b=b, mW=mW, vW=vW, mb=mb, vb=vb)


def single_runs(lib, x, y, st, wd, step0, epochs, bias, setting):
    """One sgc_train_adam_f32 call per model on its own tensors."""
    from sgc_amd import _lib
    M, K = x.shape
    B, C = st["b"].shape
    out = {k: [] for k in ("W", "b", "mW", "vW", "mb", "vb", "loss")}
    ws = torch.empty(lib.sgc_train_adam_workspace(M, K, C), dtype=torch.uint8, device=DEV)
    with knob(lib, setting):
        for i in range(B):
            t = {k: st[k][i].to(DEV).clone() for k in st}
            if not bias:
                t["b"] = t["mb"] = t["vb"] = None
            trace = torch.empty(epochs, device=DEV)
            _lib.check(lib.sgc_train_adam_f32(
                _lib.ptr(x), x.stride(0), _lib.ptr(t["W"]), _lib.ptr(t["b"]), _lib.ptr(y), M, K, C,
                _lib.ptr(t["mW"]), _lib.ptr(t["vW"]), _lib.ptr(t["mb"]), _lib.ptr(t["vb"]), step0,
                epochs, LR, BETAS[0], BETAS[1], EPS, float(wd[i]), _lib.ptr(trace), _lib.ptr(ws),
                ws.numel(), _lib.stream_handle(DEV)), "train_adam_f32")
            assert lib.sgc_get_tuning(b"adam_kernel_last") == setting
            t["loss"] = trace
            for k in out:
                if t[k] is not None:
                    out[k].append(t[k])
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in out.items() if v}


class Sweep:
    """Guarded buffers of one sgc_train_adam_sweep_f32 call."""

    def __init__(self, lib, X, y, st, wd, epochs, bias=True, pad=0):
        self.lib = lib
        self.gx, self.x = guarded_x(X, pad)
        self.y = y.to(DEV)
        self.B, self.C, self.K = st["W"].shape
        self.M = X.shape[0]
        self.g = {k: Guarded(st[k].shape, src=st[k]) for k in st if bias or "b" not in k}
        self.wd = Guarded((self.B,), src=torch.from_numpy(wd))
        self.trace = Guarded((self.B, epochs))
        self.epochs = epochs
        nbytes = lib.sgc_train_adam_sweep_workspace(self.B, self.M, self.K, self.C)
        assert nbytes > 0
        self.ws = Guarded((nbytes,), dtype=torch.uint8)

    def args(self, step0, **over):
        from sgc_amd import _lib
        g = self.g

        def p(k):
            return _lib.ptr(g[k].t) if k in g else None
        a = dict(X=_lib.ptr(self.x), ldx=self.x.stride(0), W=p("W"), b=p("b"), y=_lib.ptr(self.y),
                 B=self.B, M=self.M, K=self.K, C=self.C, mW=p("mW"), vW=p("vW"), mb=p("mb"),
                 vb=p("vb"), step0=step0, epochs=self.epochs, lr=LR, b1=BETAS[0], b2=BETAS[1],
                 eps=EPS, wd=_lib.ptr(self.wd.t), trace=_lib.ptr(self.trace.t),
                 ws=_lib.ptr(self.ws.t), ws_bytes=self.ws.t.numel(), stream=_lib.stream_handle(DEV))
        a.update(over)
        return list(a.values())

    def call(self, step0=0, **over):
        rc = self.lib.sgc_train_adam_sweep_f32(*self.args(step0, **over))
        torch.cuda.synchronize()
        return rc

    def guards(self):
        return all(g.intact() for g in (self.gx, self.wd, self.trace, self.ws, *self.g.values()))

    def result(self):
        out = {k: g.t for k, g in self.g.items()}
        out["loss"] = self.trace.t
        return out


def same_bytes(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in got:
        assert got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (what, k)


SHAPES = [(60, 500, 3), (140, 1433, 7), (120, 3703, 6), (37, 65, 17), (1, 1, 1), (313, 64, 64),
          (5, 130, 33)]
CASES = [(s, B) for s in SHAPES for B in (1, 2, 5)] + [((140, 1433, 7), 60)]
VARIANTS = [(step0, pad, bias) for step0 in (0, 7) for pad in (0, 3) for bias in (True, False)]


@pytest.mark.parametrize("form", [1, 2], ids=["fused", "split"])
@pytest.mark.parametrize("shape,B", CASES, ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple)
                         else "B%d" % v)
def test_batched_small_schedule_equals_single_calls(lib, shape, B, form):
    """step0 in {0, 7} x ldx in {K, K + 3} x bias present / absent, 3 epochs,
    on both forms of the batched launch 2."""
    M, K, C = shape
    wd = decays(B)
    for step0, pad, bias in VARIANTS:
        what = f"{shape} B={B} step0={step0} ldx=K+{pad} bias={bias} form={form}"
        X, y, st = initial(B, M, K, C, step0)
        sw = Sweep(lib, X, y, st, wd, 3, bias=bias, pad=pad)
        with form_knob(lib, form):
            assert sw.call(step0) == 0, lib.sgc_last_error()
        assert lib.sgc_get_tuning(b"adam_sweep_last") == 2, what
        assert lib.sgc_get_tuning(b"adam_sweep_form_last") == form, what
        assert sw.guards(), what
        want = single_runs(lib, sw.x, sw.y, st, wd, step0, 3, bias, 2)
        same_bytes(sw.result(), want, what)


@pytest.mark.parametrize("form", [1, 2], ids=["fused", "split"])
def test_same_weights_different_decays(lib, form):
    """B models from identical weights, each with its own decay: a kernel that
    read one decay, one bias copy or one P area for all of them would give
    equal (or wrong) results."""
    M, K, C, B = 37, 65, 17, 4
    wd = np.array([0.0, 1e-1, 1e-2, 1e-3], dtype=np.float32)
    X, y, st = initial(B, M, K, C, 0, same_weights=True)
    sw = Sweep(lib, X, y, st, wd, 3)
    with form_knob(lib, form):
        assert sw.call() == 0, lib.sgc_last_error()
    assert lib.sgc_get_tuning(b"adam_sweep_last") == 2 and sw.guards()
    got = sw.result()
    same_bytes(got, single_runs(lib, sw.x, sw.y, st, wd, 0, 3, True, 2), "same weights")
    for i in range(B):
        for j in range(i + 1, B):
            for k in ("W", "b", "mW", "vW", "mb", "vb"):
                assert not torch.equal(got[k][i], got[k][j]), (k, i, j)
    # (the first epoch's loss is taken at the shared initial weights: equal; later ones differ)
    assert len({float(v) for v in got["loss"][:, 0]}) == 1
    assert len({float(v) for v in got["loss"][:, 2]}) == B


def test_form_rule(lib):
    """"adam_sweep_form" = 0: split from 100 MB of redundant partial-logit reads
    per epoch (B n_blk^2 M C16 4 bytes), fused below (include/sgc_amd.h)."""
    M, K, C = 140, 1433, 7
    n_blk = (K + 63) // 64
    for B, form in ((5, 1), (60, 2)):
        assert (B * n_blk * n_blk * M * 16 * 4 >= 100e6) == (form == 2)
        X, y, st = initial(B, M, K, C, 0)
        sw = Sweep(lib, X, y, st, decays(B), 1)
        assert sw.call() == 0, lib.sgc_last_error()
        assert lib.sgc_get_tuning(b"adam_sweep_form") == 0
        assert lib.sgc_get_tuning(b"adam_sweep_form_last") == form and sw.guards()
    assert lib.sgc_set_tuning(b"adam_sweep_form", 3) == EINVAL


@pytest.mark.parametrize("shape,setting", [((320, 64, 3), 0), ((60, 500, 3), 1)],
                         ids=["past-row-limit", "adam_kernel-1"])
def test_general_schedule_model_by_model(lib, shape, setting):
    M, K, C = shape
    B = 3
    wd = decays(B)
    for step0, pad, bias in ((0, 0, True), (7, 3, False)):
        X, y, st = initial(B, M, K, C, step0)
        sw = Sweep(lib, X, y, st, wd, 3, bias=bias, pad=pad)
        with knob(lib, setting):
            assert sw.call(step0) == 0, lib.sgc_last_error()
        assert lib.sgc_get_tuning(b"adam_sweep_last") == 1
        assert sw.guards()
        want = single_runs(lib, sw.x, sw.y, st, wd, step0, 3, bias, 1)
        same_bytes(sw.result(), want, f"general {shape} step0={step0}")


def test_error_returns_move_nothing(lib):
    M, K, C, B = 37, 65, 17, 3
    X, y, st = initial(B, M, K, C, 0)
    sw = Sweep(lib, X, y, st, decays(B), 2)
    before = {k: g.buf.clone() for k, g in sw.g.items()}
    ws_before, trace_before = sw.ws.buf.clone(), sw.trace.buf.clone()
    cases = [("B = 0", dict(B=0), EINVAL), ("B = 4097", dict(B=4097), EINVAL),
             ("null decays", dict(wd=None), EINVAL),
             ("workspace one byte short", dict(ws_bytes=sw.ws.t.numel() - 1), ENOMEM),
             ("ldx < K", dict(ldx=K - 1), EINVAL),
             ("b without its moments", dict(mb=None), EINVAL),
             ("moments without b", dict(b=None), EINVAL)]
    assert sw.ws.t.numel() == lib.sgc_train_adam_sweep_workspace(B, M, K, C)
    for what, over, code in cases:
        assert sw.call(**over) == code, what
        assert len(lib.sgc_last_error()) > 0, what
        assert sw.guards(), what
        for k, g in sw.g.items():
            assert torch.equal(g.buf, before[k]), (what, k)
        assert torch.equal(sw.ws.buf, ws_before) and torch.equal(sw.trace.buf, trace_before), what
    assert lib.sgc_train_adam_sweep_workspace(0, M, K, C) == 0
    assert lib.sgc_train_adam_sweep_workspace(4097, M, K, C) == 0
    assert sw.call() == 0  # the same buffers are a valid call


# --- sgc_linear_eval_sweep_f32 ----------------------------------------------------------------

@pytest.mark.parametrize("shape", [(500, 1433, 7), (70, 65, 17)], ids=lambda s: "%dx%dx%d" % s)
def test_eval_sweep_equals_single_calls(lib, shape):
    from sgc_amd import _lib
    M, K, C = shape
    B = 4
    X, y, st = initial(B, M, K, C, 0)
    x, yd = X.to(DEV), y.to(DEV)
    W, b = st["W"].to(DEV), st["b"].to(DEV)
    nbytes = lib.sgc_linear_eval_workspace(M, K, C)
    names = ("pred", "confusion", "counts", "loss")
    shapes = dict(pred=(B, M), confusion=(B, C, C), counts=(B, 2), loss=(B,))
    want = {k: [] for k in names}
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for i in range(B):
        o = dict(pred=torch.empty(M, dtype=torch.int64, device=DEV),
                 confusion=torch.empty((C, C), dtype=torch.int64, device=DEV),
                 counts=torch.empty(2, dtype=torch.int64, device=DEV),
                 loss=torch.empty((), device=DEV))
        Wi, bi = W[i].clone(), b[i].clone()  # (kept alive until the call has run)
        _lib.check(lib.sgc_linear_eval_f32(
            _lib.ptr(x), x.stride(0), _lib.ptr(Wi), _lib.ptr(bi), _lib.ptr(yd),
            M, K, C, *[_lib.ptr(o[k]) for k in names], _lib.ptr(ws), nbytes,
            _lib.stream_handle(DEV)), "linear_eval_f32")
        torch.cuda.synchronize()
        for k in names:
            want[k].append(o[k])
    want = {k: torch.stack(v) for k, v in want.items()}
    assert int(want["counts"][:, 0].min()) == M
    for absent in (None,) + names:
        g = {k: Guarded(shapes[k], dtype=torch.float32 if k == "loss" else torch.int64)
             for k in names if k != absent}
        gws = Guarded((nbytes,), dtype=torch.uint8)
        rc = lib.sgc_linear_eval_sweep_f32(
            _lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(b), _lib.ptr(yd), B, M, K, C,
            *[_lib.ptr(g[k].t) if k in g else None for k in names], _lib.ptr(gws.t), nbytes,
            _lib.stream_handle(DEV))
        torch.cuda.synchronize()
        assert rc == 0, (absent, lib.sgc_last_error())
        assert gws.intact() and all(v.intact() for v in g.values()), absent
        for k in g:
            got = g[k].t
            if k == "loss":
                assert torch.equal(got.view(torch.int32), want[k].view(torch.int32)), (absent, k)
            else:
                assert torch.equal(got, want[k]), (absent, k)
    for bad_b in (0, 4097):
        assert lib.sgc_linear_eval_sweep_f32(
            _lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(b), _lib.ptr(yd), bad_b, M, K, C,
            None, None, _lib.ptr(torch.empty((B, 2), dtype=torch.int64, device=DEV)), None,
            _lib.ptr(ws), nbytes, _lib.stream_handle(DEV)) == EINVAL
        assert len(lib.sgc_last_error()) > 0


# --- the Python surface --------------------------------------------------------------------------

def build_models(n, K, C, seed):
    from sgc_amd.models import SGC
    torch.manual_seed(seed)
    return [SGC(K, C).to(DEV) for _ in range(n)]


def params_of(models, opts):
    out = []
    for m, o in zip(models, opts):
        st = o.state
        out.append(dict(W=m.W.weight.detach(), b=m.W.bias.detach(),
                        mW=st[m.W.weight]["exp_avg"], vW=st[m.W.weight]["exp_avg_sq"],
                        mb=st[m.W.bias]["exp_avg"], vb=st[m.W.bias]["exp_avg_sq"]))
        assert st[m.W.weight]["step"].tolist() == st[m.W.bias]["step"].tolist()
    return out


def test_model_bank_and_adam_sweep_equal_separate_twins(lib):
    from sgc_amd.optim import Adam
    from sgc_amd.tuning import AdamSweep, ModelBank
    M, K, C, B = 140, 1433, 7, 5
    X, _, _, y = problem(M, K, C)
    x, yd = X.to(DEV), y.to(DEV)
    wd = [float(v) for v in decays(B)]
    # the twins: the same draws, trained one by one on the small schedule
    twins = build_models(B, K, C, seed=11)
    topts = [Adam(m.parameters(), lr=LR, weight_decay=w) for m, w in zip(twins, wd)]
    with knob(lib, 2):
        traces = torch.stack([o.run_epochs(m, x, yd, 4, loss_trace=True)
                              for m, o in zip(twins, topts)])
    models = build_models(B, K, C, seed=11)
    bank = ModelBank(models)
    assert bank.weight.shape == (B, C, K) and bank.bias.shape == (B, C)
    assert all(m.W.weight.data_ptr() == bank.weight[i].data_ptr() for i, m in enumerate(models))
    sweep = AdamSweep(bank, LR, wd)
    first = sweep.run_epochs(x, yd, 2, loss_trace=True)
    assert lib.sgc_get_tuning(b"adam_sweep_last") == 2
    last = sweep.run_epochs(x, yd, 2)  # continues: step0 = 2
    torch.cuda.synchronize()
    assert first.shape == (B, 2) and last.shape == (B,)
    assert torch.equal(first, traces[:, :2]) and torch.equal(last, traces[:, 3])
    for i, (got, want) in enumerate(zip(params_of(models, sweep.optimizers),
                                        params_of(twins, topts))):
        same_bytes(got, want, f"model {i}")
        assert float(sweep.optimizers[i].state[models[i].W.weight]["step"]) == 4.0
        assert models[i].W.weight.grad is None
    # every model stays usable on its own and sees the sweep's updates
    assert torch.equal(models[2](x).as_subclass(torch.Tensor), twins[2](x).as_subclass(torch.Tensor))
    # bank.evaluate against model.evaluate
    evs = bank.evaluate(x, yd)
    assert len(evs) == B
    for m, ev in zip(models, evs):
        own = m.evaluate(x, yd)
        assert float(ev.accuracy()) == float(own.accuracy())
        assert torch.equal(ev.confusion, own.confusion)
        assert torch.equal(ev.loss.view(torch.int32), own.loss.view(torch.int32))


def test_adam_sweep_fallbacks_and_labels(lib):
    from sgc_amd.optim import Adam
    from sgc_amd.tuning import AdamSweep, ModelBank
    M, K, C, B = 37, 66, 5, 3
    X, _, _, y = problem(M, K, C)
    x16, yd = X.to(DEV).bfloat16(), y.to(DEV)
    wd = [float(v) for v in decays(B)]
    twins = build_models(B, K, C, seed=3)
    topts = [Adam(m.parameters(), lr=LR, weight_decay=w) for m, w in zip(twins, wd)]
    want = torch.stack([o.run_epochs(m, x16, yd, 3) for m, o in zip(twins, topts)])
    models = build_models(B, K, C, seed=3)
    sweep = AdamSweep(ModelBank(models), LR, wd)
    before = lib.sgc_get_tuning(b"adam_sweep_last")
    got = sweep.run_epochs(x16, yd, 3)  # bf16 features: Adam.run_epochs per model
    torch.cuda.synchronize()
    assert lib.sgc_get_tuning(b"adam_sweep_last") == before
    assert torch.equal(got, want)
    for i, (g, w) in enumerate(zip(params_of(models, sweep.optimizers), params_of(twins, topts))):
        same_bytes(g, w, f"bf16 model {i}")
    bad = yd.clone()
    bad[5] = C
    snapshot = sweep.bank.weight.clone()
    with pytest.raises(IndexError):
        sweep.run_epochs(X.to(DEV), bad, 1)
    torch.cuda.synchronize()
    assert torch.equal(sweep.bank.weight, snapshot)  # nothing moved
    assert sweep.run_epochs(X.to(DEV), yd, 0) is None


# --- the drivers -----------------------------------------------------------------------------------

def test_tuning_driver_and_tuned_from(lib, tmp_path, monkeypatch, capsys):
    import citation
    import tuning
    from planetoid_synth import write_planetoid
    from sgc_amd.models import get_model
    from sgc_amd.tuning import sample_weight_decays
    from sgc_amd.utils import load_citation, set_seed, sgc_precompute
    write_planetoid(str(tmp_path), n=1200, n_feat=300, n_class=5, n_train=100, n_test=300)
    monkeypatch.chdir(tmp_path)
    out_dir = tmp_path / "results"
    argv = ["--dataset", "synth", "--epochs", "10"]
    best, accs = tuning.main(argv + ["--max-evals", "8", "--out-dir", str(out_dir)])
    assert lib.sgc_get_tuning(b"adam_sweep_last") == 2
    lines = capsys.readouterr().out.splitlines()
    trial = [re.fullmatch(r"weight decay: (\S+) accuracy: (\d\.\d{4})", ln) for ln in lines]
    trial = [m for m in trial if m]
    assert len(trial) == 8 and len(accs) == 8
    # the same sequence of draws, trial by trial through train_regression
    args = citation.get_citation_args(argv)
    set_seed(args.seed, args.cuda)
    adj, features, labels, idx_train, idx_val, _ = load_citation(args.dataset, args.normalization,
                                                                 args.cuda)
    features, _ = sgc_precompute(features, adj, args.degree)
    wds = sample_weight_decays(8)
    models = [get_model(args.model, features.size(1), labels.max().item() + 1, args.hidden,
                        args.dropout, args.cuda) for _ in range(8)]
    want = []
    with knob(lib, 2):  # the schedule the sweep runs (bit-identical results)
        for m, w in zip(models, wds):
            _, acc, _ = citation.train_regression(
                m, features[idx_train], labels[idx_train], features[idx_val], labels[idx_val],
                args.epochs, float(w), args.lr, args.dropout, device_adam=True, device_eval=True)
            want.append(float(acc))
    for m, w, acc, got in zip(trial, wds, want, accs):
        assert m.group(1) == "{:.2e}".format(w) and m.group(2) == "{:.4f}".format(acc)
        assert got == acc
    first_best = wds[int(np.argmax(want))]  # (argmax keeps the first of a tie)
    assert "Best weight decay: {:.2e}".format(first_best) in lines
    with open(out_dir / "SGC-tuning" / "synth.txt", "rb") as f:
        saved = pickle.load(f)
    assert list(saved) == ["weight_decay"] and type(saved["weight_decay"]) is float
    assert saved["weight_decay"] == float(first_best) == best
    # citation.py --tuned-from reads it back and trains with it
    tuned = citation.main(argv + ["--tuned-from", str(out_dir), "--device-adam"])
    assert "using tuned weight decay: {}".format(saved["weight_decay"]) in capsys.readouterr().out
    explicit = citation.main(argv + ["--weight_decay", repr(saved["weight_decay"]), "--device-adam"])
    other = citation.main(argv + ["--weight_decay", "0.05", "--device-adam"])
    assert tuned == explicit
    assert "using tuned" not in capsys.readouterr().out
    print("tuned", tuned, "wd=0.05", other)
