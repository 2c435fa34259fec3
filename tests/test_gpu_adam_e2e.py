"""End-to-end: the citation driver with --device-adam (sgc_amd.optim.Adam's
run_epochs: the training loop in one host call) against the reference's own
run -- the fixture and the bound of tests/test_gpu_e2e.py."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "drivers"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "e2e_citation.json")) as f:
        return json.load(f)


@pytest.fixture
def dataset_dir(tmp_path, monkeypatch, golden):
    from planetoid_synth import write_planetoid
    write_planetoid(str(tmp_path), **dict(golden["dataset"]))
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_citation_driver_device_adam_matches_reference_accuracy(dataset_dir, golden, capsys):
    import citation
    from sgc_amd import _lib
    ref = golden["reference_citation_py"]
    argv = [a for a in ref["args"] if a != "--no-cuda"] + ["--device-adam"]
    acc_val, acc_test = citation.main(argv)
    assert _lib.load().sgc_get_tuning(b"adam_kernel_last") in (1, 2)  # the fused loop ran
    assert abs(acc_val - ref["val_acc"]) <= 0.01, (acc_val, ref["val_acc"])
    assert abs(acc_test - ref["test_acc"]) <= 0.01, (acc_test, ref["test_acc"])
    assert "train time" in capsys.readouterr().out
