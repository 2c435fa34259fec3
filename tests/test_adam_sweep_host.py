"""Weight-decay sweep checks that need no GPU: the workspace functions, the
header's declarations, sample_weight_decays, ModelBank / AdamSweep on CPU
tensors against torch.optim.Adam loops, and drivers/tuning.py with --no-cuda."""
import math
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drivers"))

CITATION_SHAPES = ((140, 1433, 7), (120, 3703, 6), (60, 500, 3))


@pytest.fixture(scope="module")
def lib():
    from sgc_amd import build
    build.build(verbose=False)
    from sgc_amd import _lib
    return _lib.load()


def test_header_declares_the_sweep_entries():
    src = open(os.path.join(ROOT, "include", "sgc_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(sgc_\w+)\s*\(", src))
    for must in ("sgc_train_adam_sweep_workspace", "sgc_train_adam_sweep_f32",
                 "sgc_linear_eval_sweep_f32"):
        assert must in names


def test_sweep_workspace(lib):
    ws = lib.sgc_train_adam_sweep_workspace
    for M, K, C in CITATION_SHAPES + ((37, 65, 17), (1, 1, 1), (313, 64, 64)):
        C16, n_blk = (C + 15) // 16 * 16, (K + 63) // 64
        area = n_blk * M * C16 * 4  # one model's partial logits (csrc/adam.hip)
        prev = 0
        for B in (1, 2, 5, 60, 4096):
            got = ws(B, M, K, C)
            assert got >= B * area and got >= prev and got > 0, (M, K, C, B)
            prev = got
    # past the small schedule's rows: the general schedule's workspace, whatever B
    assert ws(1, 320, 64, 3) == ws(60, 320, 64, 3) == lib.sgc_train_adam_workspace(320, 64, 3) > 0
    # outside coverage: 0
    for bad in ((0, 60, 500, 3), (4097, 60, 500, 3), (-1, 60, 500, 3), (3, 0, 500, 3),
                (3, 60, 0, 3), (3, 60, 500, 0), (3, 60, 500, 65)):
        assert ws(*bad) == 0, bad
    # the eval sweep uses sgc_linear_eval_workspace as it is
    assert lib.sgc_linear_eval_workspace(500, 1433, 7) > 0
    assert lib.sgc_linear_eval_workspace(500, 1433, 65) == 0
    assert lib.sgc_linear_eval_workspace(0, 1433, 7) == 0


def test_sweep_rejects_bad_arguments_on_the_host(lib):
    """Null pointers everywhere: each call stops at its first check."""
    def call(B, ldx=500, wd=None):
        return lib.sgc_train_adam_sweep_f32(None, ldx, None, None, None, B, 60, 500, 3, None, None,
                                            None, None, 0, 1, 0.2, 0.9, 0.999, 1e-8, wd, None, None,
                                            0, None)
    for B in (0, 4097):
        assert call(B) == 1 and b"B=" in lib.sgc_last_error()
    assert call(3, ldx=499) == 1 and b"ldx" in lib.sgc_last_error()
    assert call(3) == 1 and b"weight_decay_dev" in lib.sgc_last_error()
    assert lib.sgc_linear_eval_sweep_f32(None, 500, None, None, None, 0, 60, 500, 3, None, None,
                                         None, None, None, 0, None) == 1
    assert lib.sgc_get_tuning(b"adam_sweep_last") in (0, 1, 2)
    assert lib.sgc_set_tuning(b"adam_sweep_last", 1) != 0  # read-only


def test_sample_weight_decays():
    from sgc_amd.tuning import sample_weight_decays
    a, b, c = sample_weight_decays(60), sample_weight_decays(60), sample_weight_decays(60, seed=1)
    assert a.dtype == np.float64 and a.shape == (60,)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(sample_weight_decays(10), a[:10])  # a prefix of the same stream
    assert (a >= 1e-10).all() and (a <= 1e-4).all()
    assert len(sample_weight_decays(0)) == 0
    rs = np.random.RandomState(0)
    assert np.array_equal(a, np.exp(rs.uniform(math.log(1e-10), math.log(1e-4), 60)))
    # log of the draws looks uniform: n draws into k equal bins of [log low, log high] are
    # Binomial(n, 1/k) per bin, standard deviation sqrt(n (1/k) (1 - 1/k)).  Five standard
    # deviations: a normal tail of 5.7e-7 per bin, so k = 20 bins of a truly uniform sample
    # fail with probability about 1e-5; a sample uniform in the decay itself, not its log,
    # would put > 90% of the draws into the last bin.
    n, k = 10000, 20
    lo, hi = 1e-9, 1e-3
    d = sample_weight_decays(n, lo, hi, seed=5)
    assert (d >= lo).all() and (d <= hi).all()
    counts, _ = np.histogram(np.log(d), bins=k, range=(math.log(lo), math.log(hi)))
    sd = math.sqrt(n * (1 / k) * (1 - 1 / k))
    print("bin counts", counts.tolist(), "expected", n / k, "sd", round(sd, 2))
    assert counts.sum() == n
    assert np.abs(counts - n / k).max() <= 5 * sd


def torch_loop(model, x, y, epochs, lr, wd):
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
    losses = []
    for _ in range(epochs):
        model.train()
        opt.zero_grad()
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return opt, torch.stack(losses)


def test_bank_and_sweep_on_cpu_equal_torch_adam_loops():
    from sgc_amd.models import SGC
    from sgc_amd.tuning import AdamSweep, ModelBank
    M, K, C, B = 40, 33, 5, 4
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(M, K, generator=gen)
    y = torch.randint(0, C, (M,), generator=gen)
    wd = [0.0, 5e-4, 1e-6, 0.0]

    def build():
        torch.manual_seed(9)
        return [SGC(K, C) for _ in range(B)]
    twins = build()
    ref = [torch_loop(m, x, y, 4, 0.2, w) for m, w in zip(twins, wd)]
    models = build()
    bank = ModelBank(models)
    assert bank.weight.shape == (B, C, K) and bank.bias.shape == (B, C) and len(bank) == B
    assert all(m.W.weight.data_ptr() == bank.weight[i].data_ptr() for i, m in enumerate(models))
    sweep = AdamSweep(bank, 0.2, wd)
    first = sweep.run_epochs(x, y, 2, loss_trace=True)
    last = sweep.run_epochs(x, y, 2)
    assert first.shape == (B, 2) and last.shape == (B,)
    for i, (m, t, (opt, losses)) in enumerate(zip(models, twins, ref)):
        assert torch.equal(first[i], losses[:2]) and torch.equal(last[i], losses[3]), i
        assert torch.equal(m.W.weight, t.W.weight) and torch.equal(m.W.bias, t.W.bias), i
        assert torch.equal(bank.weight[i], t.W.weight.detach()), i  # the stack sees the updates
        mine = sweep.optimizers[i].state
        for p, q in ((m.W.weight, t.W.weight), (m.W.bias, t.W.bias)):
            assert torch.equal(mine[p]["exp_avg"], opt.state[q]["exp_avg"]), i
            assert torch.equal(mine[p]["exp_avg_sq"], opt.state[q]["exp_avg_sq"]), i
            assert float(mine[p]["step"]) == 4.0
    evs = bank.evaluate(x, y)
    for m, ev in zip(models, evs):
        own = m.evaluate(x, y)
        assert float(ev.accuracy()) == float(own.accuracy())
        assert torch.equal(ev.confusion, own.confusion)
    assert sweep.run_epochs(x, y, 0) is None
    bad = y.clone()
    bad[3] = C
    with pytest.raises(IndexError):
        sweep.run_epochs(x, bad, 1)
    with pytest.raises(ValueError):
        AdamSweep(bank, 0.2, wd[:2])
    with pytest.raises(TypeError):
        ModelBank([torch.nn.Linear(3, 2)])
    with pytest.raises(ValueError):
        ModelBank([SGC(3, 2), SGC(4, 2)])


def test_tuning_driver_on_the_cpu(lib, tmp_path, monkeypatch, capsys):
    import citation
    import tuning
    from planetoid_synth import write_planetoid
    write_planetoid(str(tmp_path), n=800, n_feat=40, n_class=3, n_train=30, n_test=100)
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "synth", "--no-cuda", "--epochs", "5"]
    best, accs = tuning.main(argv + ["--max-evals", "3", "--out-dir", str(tmp_path / "out")])
    lines = capsys.readouterr().out.splitlines()
    trial = [ln for ln in lines if re.fullmatch(r"weight decay: \d\.\d\de-\d\d accuracy: \d\.\d{4}", ln)]
    assert len(trial) == 3 and len(accs) == 3
    assert "Best weight decay: {:.2e}".format(best) in lines
    with open(tmp_path / "out" / "SGC-tuning" / "synth.txt", "rb") as f:
        saved = pickle.load(f)
    assert saved == {"weight_decay": best} and type(best) is float
    from sgc_amd.tuning import sample_weight_decays
    assert best == float(sample_weight_decays(3)[int(np.argmax(accs))])
    tuned = citation.main(argv + ["--tuned-from", str(tmp_path / "out")])
    assert "using tuned weight decay: {}".format(best) in capsys.readouterr().out
    assert tuned == citation.main(argv + ["--weight_decay", repr(best)])
    assert "using tuned" not in capsys.readouterr().out
