"""A numpy fp64 model of the Gram-form L-BFGS iteration of
sgc_amd/csrc/lbfgs_wide.hip, launch by launch: the ring slots, the staged pair,
the incremental Gram update, the two loops on coefficients and the direction
as one linear combination.  `MUTANTS` names one-line departures from it that
the host tests show to be caught.  Shared by tests/test_lbfgs_wide_host.py and
tests/test_gpu_lbfgs_wide.py."""
import numpy as np
import torch

MUTANTS = ("evicted_gram_kept", "stale_g_row", "stage_into_ring", "hdiag_on_reject")

# extra problems for the wide iteration (the form of test_lbfgs_host.CASES)


def _bumpy(x):
    """Non-convex: log(1 + u^2) has negative curvature beyond |u| = 1, so a step
    across it yields ys < 0 and the pair is rejected."""
    k = torch.arange(x.numel(), dtype=torch.float64)
    c = (((k * 29) % 17) / 16.0 - 0.5).to(x)
    a = (1.0 + ((k * 13) % 7) / 8.0).to(x)
    return (a * torch.log1p((x - c) ** 2)).sum()


class GramLBFGS:
    """The device state and the six launches, in fp64."""

    def __init__(self, n, m, mutant=None):
        self.n, self.m, self.mutant = n, m, mutant
        B = 2 * m + 1
        self.n_iter = self.func_evals = self.iters = self.evals = self.stop = 0
        self.h = self.head = 0
        self.S, self.Y = np.zeros((m, n)), np.zeros((m, n))
        self.ro = np.zeros(m)
        self.d, self.prev_g = np.zeros(n), np.zeros(n)
        self.s_new, self.y_new = np.zeros(n), np.zeros(n)
        self.G = np.zeros((B, B))
        self.t, self.H_diag, self.prev_loss = 0.0, 1.0, 0.0
        self.pushes = self.rejects_full = 0

    def slot(self, i, head=None):
        return ((self.head if head is None else head) + i) % self.m

    def begin_step(self):
        self.iters = self.evals = self.stop = 0

    def row(self, q, head):
        """ring row q of the scan: S then Y of each logical pair"""
        sl = self.slot(q >> 1, head)
        return (self.Y if q & 1 else self.S)[sl], (self.m + sl if q & 1 else sl)

    def iterate(self, x, loss, g, lr, max_iter, max_eval, tol_grad, tol_change):
        if self.stop:
            return
        m, h_old, head_old = self.m, self.h, self.head
        # 1 scan: the staged pair and every new dot
        self.s_new, self.y_new = self.t * self.d, g - self.prev_g
        if self.mutant == "stage_into_ring" and self.n_iter >= 1:
            sl = self.head if self.h == m else self.slot(self.h)
            self.S[sl], self.Y[sl] = self.s_new, self.y_new
        rows = [self.row(q, head_old) for q in range(2 * h_old)]
        dots = [(r @ self.s_new, r @ self.y_new, r @ g) for r, _ in rows]
        gmax, g1 = np.abs(g).max() if g.size else 0.0, np.abs(g).sum()
        tdmax = np.abs(self.t * self.d).max()
        ss, sy, yy = self.s_new @ self.s_new, self.s_new @ self.y_new, self.y_new @ self.y_new
        sg, yg, gg = self.s_new @ g, self.y_new @ g, g @ g
        # 2 coef: torch's tests (a NaN fails every comparison)
        self.func_evals += 1
        self.evals += 1
        stop = 0
        if self.evals == 1:
            if gmax <= tol_grad:
                stop = 1
        elif self.evals >= max_eval:
            stop = 3
        elif gmax <= tol_grad:
            stop = 4
        elif tdmax <= tol_change:
            stop = 6
        elif abs(loss - self.prev_loss) < tol_change:
            stop = 7
        if stop:
            self.stop = stop
            return
        self.n_iter += 1
        self.iters += 1
        first = self.n_iter == 1
        push = (not first) and sy > 1e-10
        evict = push and self.h == m
        if push:
            if evict:
                sl, self.head = self.head, (self.head + 1) % m
            else:
                sl = self.slot(self.h)
                self.h += 1
            self.H_diag = sy / yy
            self.ro[sl] = 1.0 / sy
            self.pushes += 1
        elif not first:
            if self.h == m:
                self.rejects_full += 1
            if self.mutant == "hdiag_on_reject":
                self.H_diag = sy / yy
        if first:
            self.H_diag = 1.0
        self.t = min(1.0, 1.0 / g1) * lr if first else lr
        G, ig = self.G, 2 * m
        for q, (_, R) in enumerate(rows):
            if evict and q >> 1 == 0:
                continue
            if push and not (evict and self.mutant == "evicted_gram_kept"):
                G[sl, R] = G[R, sl] = dots[q][0]
                G[m + sl, R] = G[R, m + sl] = dots[q][1]
            if push or self.mutant != "stale_g_row":
                G[ig, R] = G[R, ig] = dots[q][2]
        if push:
            G[sl, sl], G[m + sl, m + sl] = ss, yy
            G[sl, m + sl] = G[m + sl, sl] = sy
            G[ig, sl] = G[sl, ig] = sg
            G[ig, m + sl] = G[m + sl, ig] = yg
        G[ig, ig] = gg
        h = self.h
        idx = [self.slot(i) for i in range(h)] + [m + self.slot(i) for i in range(h)] + [ig]
        c = np.zeros(2 * h + 1)
        c[2 * h] = -1.0
        al = np.zeros(h)
        for i in range(h - 1, -1, -1):
            s_i = self.slot(i)
            al[i] = (c @ G[s_i, idx]) * self.ro[s_i]
            c[h + i] -= al[i]
        c *= self.H_diag
        for i in range(h):
            s_i = self.slot(i)
            be = (c @ G[m + s_i, idx]) * self.ro[s_i]
            c[i] += al[i] - be
        # 3 direct: the pair into its slot, d, prev_g
        if push:
            self.S[sl], self.Y[sl] = self.s_new, self.y_new
        d = np.zeros(self.n)
        for e in range(2 * h):
            d = d + c[e] * (self.S[idx[e]] if e < h else self.Y[idx[e] - m])
        self.d = d + c[2 * h] * g
        self.prev_g = g.copy()
        self.prev_loss = loss
        # 4 decide, 5 update
        gtd = g @ self.d
        if gtd > -tol_change:
            self.stop = 5
            return
        x += self.t * self.d
        if self.iters >= max_iter:
            self.stop = 2

    def sync_gram(self):
        """every entry from the rows as they lie (prev_g as g)"""
        rows = np.concatenate([self.S, self.Y, self.prev_g[None]])
        return rows @ rows.T

    def status(self):
        return (self.n_iter, self.func_evals, self.iters, self.evals, self.stop, self.h)


def evaluate(f, x):
    xx = torch.from_numpy(x.copy()).requires_grad_(True)
    loss = f(xx)
    (g,) = torch.autograd.grad(loss, xx, allow_unused=True)
    g = torch.zeros_like(xx) if g is None else g
    return float(loss.detach()), g.detach().numpy().copy()


def run_model(case, x0, mutant=None):
    """(x, model, [status per step]) of the case's steps: per step the reset,
    then max_iter times [closure, iterate] as the host enqueues them (closures
    after the stop are skipped: they would change nothing)."""
    opts = dict(lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                history_size=100)
    opts.update(case["opts"])
    if opts["max_eval"] is None:
        opts["max_eval"] = opts["max_iter"] * 5 // 4
    x = x0.numpy().astype(np.float64).copy()
    model = GramLBFGS(x.size, opts["history_size"], mutant)
    statuses = []
    with np.errstate(all="ignore"):
        for _ in range(case["steps"]):
            model.begin_step()
            for _it in range(opts["max_iter"]):
                if model.stop:
                    break
                loss, g = evaluate(case["f"], x)
                model.iterate(x, loss, g, opts["lr"], opts["max_iter"], opts["max_eval"],
                              opts["tolerance_grad"], opts["tolerance_change"])
            statuses.append(model.status())
    return x, model, statuses
