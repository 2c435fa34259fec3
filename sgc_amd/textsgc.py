"""TextSGC's one-hop feature precompute on the MI355X engine (SURVEY.md 8(f)
row 4) -- drop-in for sgc_precompute in the reference's
downstream/TextSGC/utils.py:131-152 (same signature, same return).

The TextSGC app (train.py:103-106) passes the normalised doc/word adjacency
`adj` and `features` = adj as a dense matrix, with degree = 1: for each
split, F = (S . features[:, idx])^T -- one SpMM whose right-hand side is the
split's columns of S -- then columns with zero range over the training rows
are dropped and every split is min/range-scaled with the training statistics.
The SpMM runs on the HIP kernel (bit-exact with torch.spmm's CPU kernel); the
transpose, min/max, filter and scaling are elementwise torch ops on the
device.  As in the reference, train stays on the device and val/test come
back to the host.

The training that follows it (train.py:52-100) is here too: `SGC`, the
bias-less classifier, and `train_linear` / `eval_linear`, whose L-BFGS steps
run on the device through sgc_amd.optim.LBFGS(wide=True).
"""
from functools import partial
from time import perf_counter

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .propagate import csr_of, spmm


class SGC(nn.Module):
    """TextSGC's classifier (reference downstream/TextSGC/models.py:6-15):
    one linear layer, no bias by default, xavier-normal weights.  On ROCm
    tensors the forward is sgc_amd.models.SGC's (the MFMA linear; its logits
    route F.cross_entropy to the HIP loss), on CPU tensors nn.Linear's."""

    def __init__(self, nfeat, nclass, bias=False):
        super().__init__()
        self.W = nn.Linear(nfeat, nclass, bias=bias)
        torch.nn.init.xavier_normal_(self.W.weight)

    def forward(self, x):
        if x.device.type == "cpu":
            return self.W(x)
        from .models import SGCLogits, _LinearMFMA
        return _LinearMFMA.apply(x, self.W.weight, self.W.bias).as_subclass(SGCLogits)


def _criterion(binary):
    if not binary:
        return partial(F.log_softmax, dim=1), F.nll_loss
    return torch.sigmoid, F.binary_cross_entropy


def train_linear(model, feat_dict, label_dict, weight_decay, epochs=3, binary=False):
    """(val_acc, model, train_time) of the reference's train_linear
    (downstream/TextSGC/train.py:52-78), with what that file reads from
    globals (label_dict, args.epochs) passed in: `epochs` steps of
    optim.LBFGS(model.parameters()) at torch's defaults on the closure
    criterion(act(model(train))) + 0.5 * weight_decay * (W ** 2).sum(), then
    eval_linear on the validation split.  The splits are moved to the model's
    device (the reference's .cuda()).

    On a ROCm model the multi-class training is one
    LBFGS(wide=True).run_steps(model, x, y, epochs, l2=weight_decay): the
    closures and the L-BFGS iterations are enqueued by one host call.
    binary=True (MR: one output, sigmoid + binary_cross_entropy) keeps the
    reference closure in torch ops and drives it through
    LBFGS(wide=True).step, the device optimiser.  A CPU model runs
    torch.optim.LBFGS on the reference closure, as --no-cuda does."""
    from .optim import LBFGS
    act, criterion = _criterion(binary)
    dev = model.W.weight.device
    x = feat_dict["train"].to(dev)
    y = label_dict["train"].to(dev)
    on_gpu = dev.type == "cuda"
    if on_gpu:
        optimizer = LBFGS(model.parameters(), wide=True)
        torch.cuda.synchronize(dev)
    else:
        optimizer = torch.optim.LBFGS(model.parameters())
    start = perf_counter()
    if on_gpu and not binary:
        optimizer.run_steps(model, x, y, epochs, l2=weight_decay)
    else:
        model.train()
        for _ in range(epochs):
            def closure():
                optimizer.zero_grad()
                output = model(x).squeeze()
                l2_reg = 0.5 * weight_decay * (model.W.weight ** 2).sum()
                loss = criterion(act(output), y) + l2_reg
                loss.backward()
                return loss

            optimizer.step(closure)
    if on_gpu:
        torch.cuda.synchronize(dev)
    train_time = perf_counter() - start
    val_res = eval_linear(model, feat_dict["val"].to(dev), label_dict["val"].to(dev), binary)
    return val_res["accuracy"], model, train_time


def eval_linear(model, features, label, binary=False):
    """{'loss', 'accuracy'} of the reference's eval_linear (train.py:80-100)."""
    model.eval()
    act, criterion = _criterion(binary)
    with torch.no_grad():
        output = model(features).squeeze()
        loss = criterion(act(output), label)
        if not binary:
            predict_class = output.max(1)[1]
        else:
            predict_class = act(output).gt(0.5).float()
        correct = torch.eq(predict_class, label).long().sum().item()
        acc = correct / predict_class.size(0)
    return {"loss": loss.item(), "accuracy": acc}


def sparse_to_torch_sparse(sparse_mx, device="cuda"):
    """scipy -> torch sparse COO fp32 (reference TextSGC utils.py:103-118)."""
    coo = sparse_mx.tocoo().astype(np.float32)
    indices = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
    return torch.sparse_coo_tensor(indices, torch.from_numpy(coo.data),
                                   torch.Size(coo.shape)).to(device)


def sparse_to_torch_dense(sparse, device="cuda"):
    """(reference TextSGC utils.py:120-123)"""
    return torch.from_numpy(np.asarray(sparse.todense()).astype(np.float32)).to(device=device)


def sgc_precompute(adj, features, degree, index_dict):
    """(feat_dict, seconds) exactly as the reference's TextSGC sgc_precompute;
    adj must be on the ROCm device (the reference moves it there too)."""
    assert degree == 1, "Only supporting degree 2 now"  # the reference's message
    dev = adj.device
    if dev.type != "cuda":
        raise RuntimeError("sgc_amd.textsgc: adj must be on the ROCm device (no CPU fallback)")
    torch.cuda.synchronize(dev)
    start = perf_counter()
    csr = csr_of(adj)

    def hop(idx):
        X = features[:, idx].to(dev, non_blocking=True).contiguous()
        return spmm(csr, X).t()

    feat_dict = {}
    train_feats = hop(index_dict["train"])
    train_feats_max, _ = train_feats.max(dim=0, keepdim=True)
    train_feats_min, _ = train_feats.min(dim=0, keepdim=True)
    train_feats_range = train_feats_max - train_feats_min
    useful = train_feats_range.squeeze().gt(0).nonzero().squeeze()
    train_feats = train_feats[:, useful]
    train_feats_range = train_feats_range[:, useful]
    train_feats_min = train_feats_min[:, useful]
    feat_dict["train"] = (train_feats - train_feats_min) / train_feats_range
    for phase in ["test", "val"]:
        feats = hop(index_dict[phase])[:, useful]
        feat_dict[phase] = ((feats - train_feats_min) / train_feats_range).cpu()
    torch.cuda.synchronize(dev)
    return feat_dict, perf_counter() - start
