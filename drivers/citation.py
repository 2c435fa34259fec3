"""Citation-network driver on the MI355X engine -- counterpart of the
reference's citation.py (same flags via get_citation_args, same output
lines), reading Planetoid files from ./data like the reference.

    python drivers/citation.py --dataset cora [--tuned] [--degree 2] [--epochs 100]
                               [--feature-dtype {float32,bfloat16,float16}] [--device-adam]
                               [--device-eval] [--tuned-from DIR]

Flow (reference citation.py:14-70): seed -> load_citation -> SGC model
(created before the precompute, so the RNG draws for W match) ->
sgc_precompute on the GPU -> Adam over the training rows -> accuracy.
--tuned uses the tuned weight decays of the reference's SGC-tuning/ results
(values recorded in SURVEY.md section 2, row 11; the pickled files are not
read).  --feature-dtype (this driver's own flag, default float32) casts the
loaded features once: the propagated features, the training rows and the
evaluation rows stay in that type, the weights and logits in float32.
--device-adam (also this driver's own) trains with sgc_amd.optim.Adam's
run_epochs: the same loop, enqueued on the GPU by one host call; without it
the loop below runs through torch.optim.Adam as before.  The two combine:
--feature-dtype bfloat16 --device-adam trains on the 16-bit rows in one host
call too (sgc_train_adam_x16; an odd feature count such as Cora's 1433 costs
one even-pitch copy of the training rows per call).
--device-eval (this driver's own as well) takes the validation and the test
accuracy from model.evaluate: one launch chain per split that reads the rows
once and leaves the counts on the GPU, in place of accuracy(model(x), y); the
printed lines keep their format and values.
--tuned-from DIR (this driver's own too) reads the weight decay from
DIR/{model}-tuning/{dataset}.txt, the pickle drivers/tuning.py writes, as the
reference's --tuned reads its result files (citation.py:17-21), and prints
the same "using tuned weight decay:" line; it takes precedence over --tuned.
"""
import argparse
import os
import pickle as pkl
import sys
from time import perf_counter

import torch
import torch.nn.functional as F
import torch.optim as optim

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd.args import get_citation_args  # noqa: E402
from sgc_amd.metrics import accuracy  # noqa: E402
from sgc_amd.models import get_model  # noqa: E402
from sgc_amd.utils import load_citation, set_seed, sgc_precompute  # noqa: E402

FEATURE_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
TUNED_WEIGHT_DECAY = {"cora": 1.3027e-05, "citeseer": 2.3546e-05, "pubmed": 7.4039e-05}


def train_regression(model, train_features, train_labels, val_features, val_labels,
                     epochs, weight_decay, lr, dropout, device_adam=False, device_eval=False):
    if device_adam:  # the whole loop below in one host call (sgc_amd/optim.py)
        from sgc_amd.optim import Adam
        optimizer = Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
        t = perf_counter()
        optimizer.run_epochs(model, train_features, train_labels, epochs)
        if train_features.device.type == "cuda":
            torch.cuda.synchronize(train_features.device)  # the epochs are only enqueued
    else:
        optimizer = optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
        t = perf_counter()
        for _ in range(epochs):
            model.train()
            optimizer.zero_grad()
            loss = F.cross_entropy(model(train_features), train_labels)
            loss.backward()
            optimizer.step()
    train_time = perf_counter() - t
    with torch.no_grad():
        model.eval()
        if device_eval:
            acc_val = model.evaluate(val_features, val_labels).accuracy()
        else:
            acc_val = accuracy(model(val_features), val_labels)
    return model, acc_val, train_time


def test_regression(model, test_features, test_labels, device_eval=False):
    model.eval()
    if device_eval:  # the counts on the GPU, no logits (SGC.evaluate)
        return model.evaluate(test_features, test_labels).accuracy()
    return accuracy(model(test_features), test_labels)


def parse_own(argv=None):
    """This driver's own flags (the rest are get_citation_args')."""
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--feature-dtype", choices=sorted(FEATURE_DTYPES), default="float32",
                     help="storage type of the features; with --device-adam the 16-bit rows "
                          "train in one host call as well")
    own.add_argument("--device-adam", action="store_true", default=False,
                     help="train with sgc_amd.optim.Adam.run_epochs (the epochs in one host call, "
                          "on float32, bfloat16 or float16 features)")
    own.add_argument("--device-eval", action="store_true", default=False,
                     help="take the validation and test accuracy from model.evaluate (fused "
                          "forward, argmax and counts on the GPU; no logits matrix)")
    own.add_argument("--tuned-from", metavar="DIR", default=None,
                     help="read the weight decay from DIR/{model}-tuning/{dataset}.txt (written "
                          "by drivers/tuning.py)")
    return own.parse_known_args(argv)[0]


def main(argv=None):
    args = get_citation_args(argv)
    own_args = parse_own(argv)
    feature_dtype = FEATURE_DTYPES[own_args.feature_dtype]
    if own_args.tuned_from is not None:  # (reference citation.py:17-21, on this engine's result)
        if args.model != "SGC":
            raise NotImplementedError("tuned hyper-parameters exist for SGC only")
        path = os.path.join(own_args.tuned_from, "{}-tuning".format(args.model),
                            "{}.txt".format(args.dataset))
        with open(path, "rb") as f:
            args.weight_decay = pkl.load(f)["weight_decay"]
        print("using tuned weight decay: {}".format(args.weight_decay))
    elif args.tuned:
        if args.model != "SGC":
            raise NotImplementedError("tuned hyper-parameters exist for SGC only")
        args.weight_decay = TUNED_WEIGHT_DECAY[args.dataset]
        print("using tuned weight decay: {}".format(args.weight_decay))
    set_seed(args.seed, args.cuda)
    adj, features, labels, idx_train, idx_val, idx_test = load_citation(
        args.dataset, args.normalization, args.cuda)
    model = get_model(args.model, features.size(1), labels.max().item() + 1, args.hidden,
                      args.dropout, args.cuda)
    if feature_dtype != torch.float32:
        features = features.to(feature_dtype)
    features, precompute_time = sgc_precompute(features, adj, args.degree)
    print("{:.4f}s".format(precompute_time))
    model, acc_val, train_time = train_regression(
        model, features[idx_train], labels[idx_train], features[idx_val], labels[idx_val],
        args.epochs, args.weight_decay, args.lr, args.dropout,
        **({"device_adam": True} if own_args.device_adam else {}),  # (absent: the call as before)
        **({"device_eval": True} if own_args.device_eval else {}))
    acc_test = test_regression(model, features[idx_test], labels[idx_test],
                               **({"device_eval": True} if own_args.device_eval else {}))
    print("Validation Accuracy: {:.4f} Test Accuracy: {:.4f}".format(acc_val, acc_test))
    print("Pre-compute time: {:.4f}s, train time: {:.4f}s, total: {:.4f}s".format(
        precompute_time, train_time, precompute_time + train_time))
    return float(acc_val), float(acc_test)


if __name__ == "__main__":
    main()
