"""plh_lm_step and fit_ensemble on the GPU, measured (reported, not gated: the entry is justified by the C ABI, by bounds and by scaling, not by its time).

  python tools/lm_bench.py [--out profiles/lm_fit.json] [--cells 8192] [--points 200] [--reps 9] [--max-iter 12]

Shape: the C4 shard (8192 jittered cells, 1C discharge), the seven sweep parameters, device=True, 200 measurement times shared by all cells; the data are cell 0's curve plus
2 mV of noise.  Recorded:
  lm_step            one plh_lm_step (phase STEP, every cell judging a trial and proposing the next) on the fit ens.lsq left in HBM: HIP events around the call, median of
                     --reps after one warm-up, the per-cell state restored before every repetition (outside the timed window) so that every repetition does the same work
  torch_composition  the same step composed from torch as INTEGRATION.md had it before plh_lm_step (diag_embed, linalg.solve, where): no bounds, no scaling, no failure
                     handling; timed the same way, alternating with lm_step
  sens_integration   the sensitivity kernel of one iteration (plh_last_kernel_ms)
  fit                one fit_ensemble from starts at 2^(+-0.25) of the truth in the seven keys: per iteration the number of cells still running before it, and from that the
                     share of cell-integrations spent on cells already done (the ensemble is not compacted)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lsq_bench import spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_fit.json"))
    ap.add_argument("--cells", type=int, default=8192)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-iter", type=int, default=12)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tools/lm_bench.py measures on a GPU"
    import pkgload
    pkg = pkgload.load()
    cap = pkg._capi
    p = pkg.petlion(pkg.LCO)
    n, n_q = a.cells, a.points
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    k = len(keys)
    cols = np.ascontiguousarray([p.θ_keys.index(x) for x in keys], dtype=np.int32)
    cfg = pkg.configs.c4(p, n)
    sim = lambda th: pkg.simulate_ensemble(p, th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys)
    Th = torch.from_numpy(cfg["theta"]).cuda()
    ens = sim(Th)
    torch.cuda.synchronize()
    t_end = float(ens.run_info["t_end"][:, -1].min())
    tq = np.linspace(0.0, t_end, n_q)
    rng = np.random.default_rng(0)
    data = ens(tq, fields="V").V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()
    w = torch.full((n_q,), 1 / 2e-3, dtype=torch.float64, device="cuda")
    fit0 = ens.lsq(tq, data, weights=w)
    lib, h = p._lib, p._h
    tf = np.full(k, cap.LM_LOG, np.int32)
    mk = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")
    st = dict(theta_cur=mk(n, k), cost_cur=mk(n), grad_cur=mk(n, k), JtJ_cur=mk(n, k, k), lam=mk(n), pred=mk(n), state=mk(n, dt=torch.int32), n_accept=mk(n, dt=torch.int32), n_reject=mk(n, dt=torch.int32))
    nrun = mk(1, dt=torch.int32)
    theta = Th.clone()

    def step(fit, phase):
        cap.check(lib, lib.plh_lm_step(h, n, theta.shape[1], theta.data_ptr(), k, cols.ctypes.data, tf.ctypes.data, None, None, 0, fit.cost.data_ptr(), fit.grad.data_ptr(), fit.JtJ.data_ptr(),
                                       fit.status.data_ptr(), *[st[x].data_ptr() for x in st], None, phase, nrun.data_ptr(), cap.PLH_DEVICE, None), "plh_lm_step")

    step(fit0, cap.LM_FIRST)                                                    # theta now holds every cell's first trial
    fit1 = sim(theta).lsq(tq, data, weights=w)                                  # the fit of the trials: what a STEP call consumes
    torch.cuda.synchronize()
    keep = {x: v.clone() for x, v in st.items()}
    keep_theta = theta.clone()

    def restore():
        for x, v in keep.items():
            st[x].copy_(v)
        theta.copy_(keep_theta)

    lam = torch.full((n,), 1e-3, dtype=torch.float64, device="cuda")
    cost_cur = fit0.cost

    def torch_step():                                                           # INTEGRATION.md's six lines before plh_lm_step, for the same inputs
        A = fit1.JtJ + lam[:, None, None] * torch.diag_embed(torch.diagonal(fit1.JtJ, dim1=1, dim2=2))
        th = keep_theta.clone()
        th[:, cols] -= torch.linalg.solve(A, fit1.grad)
        return th, torch.where(fit1.cost < cost_cur, lam / 3, lam * 3)

    step(fit1, cap.LM_STEP); torch_step(); torch.cuda.synchronize()             # warm-up of both
    running_after = int(nrun.cpu()[0])
    accepted = int((st["n_accept"] == 1).sum().cpu())
    ms_k, ms_t = [], []
    for _ in range(a.reps):
        restore(); torch.cuda.synchronize()
        ms_k.append(timed(lambda: step(fit1, cap.LM_STEP))[0])
        ms_t.append(timed(torch_step)[0])
    ms_s = []
    for _ in range(3):
        e = sim(Th); torch.cuda.synchronize(); ms_s.append(float(e.kernel_ms))
    # one whole fit: cells still running before every iteration
    start = Th.clone()
    start[:, cols] *= torch.from_numpy(2.0 ** rng.uniform(-0.25, 0.25, size=(n, k))).cuda()
    res = pkg.fit_ensemble(p, start, cfg["protocol"], keys, tq, data, w, SOC=cfg["SOC"], max_points=cfg["max_points"], transform={x: "log" for x in keys}, max_iter=a.max_iter, device=True, history=True)
    before = [n] + [r["n_running"] for r in res.history[:-1]]
    done_share = float(sum(n - b for b in before) / (n * len(before)))
    names = cap.LM_STATE_NAMES
    state = res.state.cpu().numpy()
    rec = {"cells": n, "n_q": n_q, "keys": keys, "transform": "log",
           "lm_step": dict(spread(ms_k), phase="STEP", cells_accepting=accepted, cells_running_after=running_after),
           "torch_composition": dict(spread(ms_t), what="diag_embed + linalg.solve + where on the same fit: no bounds, no scaling, no failure handling"),
           "lm_step_over_torch_composition": float(np.median(ms_k) / np.median(ms_t)),
           "sens_integration": spread(ms_s), "lm_step_over_sens_integration": float(np.median(ms_k) / np.median(ms_s)),
           "fit": {"max_iter": a.max_iter, "integrations": res.n_iter, "cells_running_before_each": before, "share_of_cell_integrations_on_done_cells": done_share,
                   "final_states": {names[s]: int((state == s).sum()) for s in range(len(names))}},
           "build_info": p._lib.plh_build_info().decode()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps({x: rec[x] for x in ("lm_step", "torch_composition", "lm_step_over_torch_composition", "sens_integration", "fit")}))


if __name__ == "__main__":
    main()
