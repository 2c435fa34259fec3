"""Weight-decay search for the citation networks on the MI355X engine --
counterpart of the reference's tuning.py (same flags via get_citation_args,
same output lines, same result file).

    python drivers/tuning.py --dataset cora [--max-evals 60] [--sweep-seed 0]
                             [--feature-dtype {float32,bfloat16,float16}] [--out-dir .]

Flow (reference tuning.py:14-38): seed -> load_citation -> one sgc_precompute
-> `--max-evals` models built by successive get_model calls (the RNG draws the
reference's sequential trials would make) -> one AdamSweep.run_epochs on
features[idx_train] (every trial's `--epochs` epochs in one host call on
float32 features) -> one ModelBank.evaluate on the validation rows.  It
prints one "weight decay: ... accuracy: ..." line per trial and "Best weight
decay: ...", and pickles {"weight_decay": best} to
{out-dir}/{model}-tuning/{dataset}.txt, which `drivers/citation.py
--tuned-from {out-dir}` reads as the reference's `citation.py --tuned` reads
its own.  A tie on accuracy keeps the first trial.

This is a random search in one batch, not the reference's TPE: the decays are
`--max-evals` log-uniform draws over the reference's space [1e-10, 1e-4]
(sgc_amd.tuning.sample_weight_decays, seeded by --sweep-seed).  hyperopt's TPE
proposes each trial from the results of the trials before it -- the sequential
loop that the batch replaces.
"""
import argparse
import os
import pickle as pkl
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd.args import get_citation_args  # noqa: E402
from sgc_amd.models import get_model  # noqa: E402
from sgc_amd.tuning import AdamSweep, ModelBank, sample_weight_decays  # noqa: E402
from sgc_amd.utils import load_citation, set_seed, sgc_precompute  # noqa: E402

FEATURE_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def parse_own(argv=None):
    """This driver's own flags (the rest are get_citation_args')."""
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--max-evals", type=int, default=60,
                     help="number of trials (the reference's fmin(max_evals=60))")
    own.add_argument("--sweep-seed", type=int, default=0,
                     help="seed of the log-uniform weight-decay draws")
    own.add_argument("--feature-dtype", choices=sorted(FEATURE_DTYPES), default="float32",
                     help="storage type of the features (16-bit features train model by model)")
    own.add_argument("--out-dir", default=".",
                     help="where {model}-tuning/{dataset}.txt is written")
    return own.parse_known_args(argv)[0]


def main(argv=None):
    args = get_citation_args(argv)
    own_args = parse_own(argv)
    if args.model != "SGC":
        raise NotImplementedError("the weight-decay search exists for SGC only")
    if own_args.max_evals < 1:
        raise ValueError("--max-evals must be >= 1")
    set_seed(args.seed, args.cuda)
    adj, features, labels, idx_train, idx_val, idx_test = load_citation(
        args.dataset, args.normalization, args.cuda)
    feature_dtype = FEATURE_DTYPES[own_args.feature_dtype]
    if feature_dtype != torch.float32:
        features = features.to(feature_dtype)
    features, precompute_time = sgc_precompute(features, adj, args.degree)
    nclass = labels.max().item() + 1
    decays = sample_weight_decays(own_args.max_evals, seed=own_args.sweep_seed)
    models = [get_model(args.model, features.size(1), nclass, args.hidden, args.dropout, args.cuda)
              for _ in range(own_args.max_evals)]
    bank = ModelBank(models)
    sweep = AdamSweep(bank, lr=args.lr, weight_decays=decays)
    sweep.run_epochs(features[idx_train], labels[idx_train], args.epochs)
    for m in models:
        m.eval()
    evals = bank.evaluate(features[idx_val], labels[idx_val])
    accs = torch.stack([ev.accuracy() for ev in evals]).cpu().tolist()  # one read-back
    best_i = 0
    for i, (wd, acc) in enumerate(zip(decays, accs)):
        print("weight decay: {:.2e} ".format(wd) + "accuracy: {:.4f}".format(acc))
        if acc > accs[best_i]:
            best_i = i
    best = {"weight_decay": float(decays[best_i])}
    print("Best weight decay: {:.2e}".format(best["weight_decay"]))
    out = os.path.join(own_args.out_dir, "{}-tuning".format(args.model))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "{}.txt".format(args.dataset))
    with open(path, "wb") as f:
        pkl.dump(best, f)
    return best["weight_decay"], accs


if __name__ == "__main__":
    main()
