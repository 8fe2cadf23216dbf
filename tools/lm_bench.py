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
                     share of cell-integrations spent on cells already done (the ensemble is not compacted)

  python tools/lm_bench.py --groups [--out profiles/lm_groups.json]          parameters shared by groups of cells (plh_lsq_group, plh_group_scatter, fit_ensemble(groups=...))
  group_calls        plh_lsq_group + plh_group_scatter on the fit ens.lsq left in HBM (the C4-shard shape, seven keys), HIP events around the two calls, median of --reps after a
                     warm-up; 2048 groups of 4 and 1 group of 8192; alternating in the same process with the torch composition of the same result (index_add_ /
                     repeat_interleave: another order of summation, no definition of the bits)
  fits               the seven keys from starts at 2^(+-0.25) of the truth, max_iter as above: 2048 groups of 4 members at 0.5C / 1C / 2C / 3C against 8192 single 1C cells,
                     the same number of data per problem (200: the groups' members have 50 each) with 2 mV of noise; the final states, cond of the final JtJ in log
                     parameters, and how far the best point is from the truth
  bench_c2_same_box  with --c2-line FILE: the line `bench.py --gpus 1` printed on the same box (the integrator is untouched by the grouping)

  python tools/lm_bench.py --cov [--out profiles/fit_cov.json]               covariances and identifiability of the fitted problems (plh_fit_cov)
  fit_cov            one plh_fit_cov on the state plh_lm_step (FIRST) left in HBM for the C4-shard shape (8192 problems, seven LOG keys, n_data = 200) and on the same fit summed
                     into 2048 groups of 4 (n_data = 800): HIP events around the call, median of --reps after a warm-up; alternating in the same process with the torch
                     composition of the same numbers (scaling, normalisation, linalg.cholesky_ex, cholesky_inverse, linalg.eigh on the normalised matrix: no bounds, no active
                     set, no unseen keys, no status); both as a share of the sensitivity integration; bench_c2_same_box as above"""
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
    ap.add_argument("--groups", action="store_true", help="measure the grouped calls and the grouped fit instead (default --out: profiles/lm_groups.json)")
    ap.add_argument("--cov", action="store_true", help="measure plh_fit_cov instead (default --out: profiles/fit_cov.json)")
    ap.add_argument("--c2-line", default=None, help="--groups / --cov: a file whose last line is the JSON line `bench.py --gpus 1` printed on the same box; kept in the record as bench_c2_same_box")
    a = ap.parse_args()
    if a.groups:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "lm_groups.json")
        return main_groups(a)
    if a.cov:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "fit_cov.json")
        return main_cov(a)
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


def main_groups(a):
    import torch
    assert torch.cuda.is_available(), "tools/lm_bench.py measures on a GPU"
    import pkgload
    pkg = pkgload.load()
    cap = pkg._capi
    p = pkg.petlion(pkg.LCO)
    lib, h = p._lib, p._h
    n, n_q = a.cells, a.points
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    k = len(keys)
    cols = np.ascontiguousarray([p.θ_keys.index(x) for x in keys], dtype=np.int32)
    cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
    nth = len(p.θ_keys)
    rng = np.random.default_rng(0)

    # ---- (a) the two calls on the C4-shard fit
    cfg = pkg.configs.c4(p, n)
    Th = torch.from_numpy(cfg["theta"]).cuda()
    ens = pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys)
    torch.cuda.synchronize()
    tq = np.linspace(0.0, float(ens.run_info["t_end"][:, -1].min()), n_q)
    data = ens(tq, fields="V").V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()
    w = torch.full((n_q,), 1 / 2e-3, dtype=torch.float64, device="cuda")
    fit = ens.lsq(tq, data, weights=w)
    ms_s = []
    for _ in range(3):
        e = pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys); torch.cuda.synchronize(); ms_s.append(float(e.kernel_ms))
    calls = {}
    for name, sizes in (("%d_groups_of_4" % (n // 4), [4] * (n // 4)), ("1_group_of_%d" % n, [n])):
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int32)
        ng = len(sizes)
        lab = torch.from_numpy(np.repeat(np.arange(ng), sizes)).cuda()
        counts = torch.from_numpy(np.asarray(sizes)).cuda()
        mk = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")
        g = dict(cost=mk(ng), grad=mk(ng, k), JtJ=mk(ng, k, k), status=mk(ng, dt=torch.int32))
        g_theta, theta = Th[torch.from_numpy(off[:-1].astype(np.int64)).cuda()].contiguous(), Th.clone()
        theta2 = Th.clone()

        def ours():
            cap.check(lib, lib.plh_lsq_group(h, n, ng, off.ctypes.data, k, fit.cost.data_ptr(), fit.grad.data_ptr(), fit.JtJ.data_ptr(), fit.status.data_ptr(),
                                             g["cost"].data_ptr(), g["grad"].data_ptr(), g["JtJ"].data_ptr(), g["status"].data_ptr(), cap.PLH_DEVICE, None), "plh_lsq_group")
            cap.check(lib, lib.plh_group_scatter(h, n, ng, off.ctypes.data, nth, k, cols.ctypes.data, g_theta.data_ptr(), theta.data_ptr(), cap.PLH_DEVICE, None), "plh_group_scatter")

        def torch_composition():
            c = mk(ng).index_add_(0, lab, fit.cost); gr = mk(ng, k).index_add_(0, lab, fit.grad); H = mk(ng, k, k).index_add_(0, lab, fit.JtJ)
            s = mk(ng, dt=torch.int32).index_add_(0, lab, (fit.status != 0).to(torch.int32)) > 0
            theta2[:, cols_t] = torch.repeat_interleave(g_theta[:, cols_t], counts, dim=0)
            return c, gr, H, s

        ours(); tc = torch_composition(); torch.cuda.synchronize()                # warm-up of both
        rel = float(((tc[2] - g["JtJ"]).abs().amax() / g["JtJ"].abs().amax()).cpu())
        assert torch.equal(theta, theta2) and rel < 1e-9, rel
        ms_k, ms_t = [], []
        for _ in range(a.reps):
            ms_k.append(timed(ours)[0])
            ms_t.append(timed(torch_composition)[0])
        calls[name] = {"groups": ng, "plh_lsq_group_and_scatter": spread(ms_k), "torch_composition": spread(ms_t), "ours_over_torch_composition": float(np.median(ms_k) / np.median(ms_t)),
                       "ours_over_sens_integration": float(np.median(ms_k) / np.median(ms_s)), "JtJ_rel_difference_to_torch_composition": rel}

    # ---- (b) the fit the grouping is for
    rates = [0.5, 1.0, 2.0, 3.0]
    truth = pkg.theta_matrix(p, 1)
    names = cap.LM_STATE_NAMES
    tf = {x: "log" for x in keys}
    t_end = {}
    for r in rates:
        e = pkg.simulate_ensemble(p, torch.from_numpy(truth).cuda(), [{"I": -r}], SOC=1.0, device=True, max_points=512)
        torch.cuda.synchronize()
        t_end[r] = float(e.run_info["t_end"][0, -1])

    def problem(member_rates, n_groups):
        """n_groups problems whose members run at member_rates; n_q data per problem, shared evenly among the members"""
        m = len(member_rates)
        per = n_q // m
        tq = np.concatenate([np.linspace(0.0, 0.95 * t_end[r], per) for r in member_rates])
        I = np.tile([-r for r in member_rates], n_groups)
        proto = [{"I": I}]
        Th1 = torch.from_numpy(np.repeat(truth, m, axis=0)).cuda()
        e = pkg.simulate_ensemble(p, Th1, [{"I": np.asarray([-r for r in member_rates])}], SOC=1.0, device=True, max_points=512)
        V = e(tq, fields="V").V.cpu().numpy()                                   # [m, n_q]: the truth at every member's rate
        wm = np.zeros((m, len(tq)))
        for j in range(m):
            wm[j, j * per:(j + 1) * per] = 1 / 2e-3
        V = np.where(wm > 0, V, 0.0)
        data = np.tile(V, (n_groups, 1)) + 2e-3 * rng.standard_normal((n_groups * m, len(tq)))
        start = np.repeat(truth, n_groups * m, axis=0)
        start[:, cols] *= np.repeat(2.0 ** rng.uniform(-0.25, 0.25, size=(n_groups, k)), m, axis=0)
        return proto, tq, torch.from_numpy(data).cuda(), torch.from_numpy(np.tile(wm, (n_groups, 1))).cuda(), torch.from_numpy(start).cuda(), m

    def run(member_rates, n_groups, grouped):
        proto, tq, data, wts, start, m = problem(member_rates, n_groups)
        groups = np.repeat(np.arange(n_groups), m) if grouped else None
        t0 = timed(lambda: pkg.fit_ensemble(p, start, proto, keys, tq, data, wts, SOC=1.0, max_points=512, transform=tf, max_iter=a.max_iter, device=True, history=False, groups=groups))
        ms, res = t0
        state = res.state.cpu().numpy()
        th = res.theta.cpu().numpy()[::m][:, cols]                              # a group's point: its first member's
        s = th[:, :, None] * th[:, None, :]
        H = res.JtJ.cpu().numpy() * s                                           # in log parameters
        ok = np.isfinite(H).all(axis=(1, 2))
        cond = np.full(len(H), np.nan)
        cond[ok] = np.linalg.cond(H[ok])
        err = np.abs(th / truth[0, cols] - 1).max(axis=1)
        q = lambda x: {"p10": float(np.nanpercentile(x, 10)), "median": float(np.nanmedian(x)), "p90": float(np.nanpercentile(x, 90))}
        conv = int(np.isin(state, (cap.LM_CONV_F, cap.LM_CONV_X, cap.LM_CONV_G)).sum())
        return {"problems": int(len(state)), "cells": int(len(state) * m), "members_at_C_rates": member_rates, "data_per_problem": int(m * (n_q // m)), "integrations": res.n_iter,
                "fit_ms": float(ms), "converged": conv, "stalled": int((state == cap.LM_STALLED).sum()), "still_descending_at_max_iter": int((state == cap.LM_MAXIT).sum()),
                "final_states": {names[x]: int((state == x).sum()) for x in range(len(names))}, "cond_JtJ_log_parameters": q(cond),
                "max_over_keys_of_abs_theta_over_truth_minus_1": q(err), "cost": q(res.cost.cpu().numpy())}

    fits = {"groups_of_4": run(rates, n // 4, True), "single_1C_cells": run([1.0], n, False)}
    rec = {"cells": n, "n_q": n_q, "keys": keys, "transform": "log", "max_iter": a.max_iter, "sens_integration": spread(ms_s), "group_calls": calls, "fits": fits,
           "build_info": p._lib.plh_build_info().decode()}
    if a.c2_line:                                                               # the integrator of the same binary on the same box
        b = json.loads([line for line in open(a.c2_line) if line.startswith('{"metric"')][-1])
        rec["bench_c2_same_box"] = dict({x: b[x] for x in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")}, kernel_ms_avg=b["roofline"]["kernel_ms_avg"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


def main_cov(a):
    import torch
    assert torch.cuda.is_available(), "tools/lm_bench.py measures on a GPU"
    import pkgload
    pkg = pkgload.load()
    cap = pkg._capi
    p = pkg.petlion(pkg.LCO)
    n, n_q = a.cells, a.points
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    k = len(keys)
    cols_t = torch.from_numpy(np.asarray([p.θ_keys.index(x) for x in keys], dtype=np.int64)).cuda()
    rng = np.random.default_rng(0)
    cfg = pkg.configs.c4(p, n)
    Th = torch.from_numpy(cfg["theta"]).cuda()
    sim = lambda: pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys)
    ens = sim()
    torch.cuda.synchronize()
    tq = np.linspace(0.0, float(ens.run_info["t_end"][:, -1].min()), n_q)
    data = ens(tq, fields="V").V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()
    w = torch.full((n_q,), 1 / 2e-3, dtype=torch.float64, device="cuda")
    fit = ens.lsq(tq, data, weights=w)
    ms_s = []
    for _ in range(3):
        e = sim(); torch.cuda.synchronize(); ms_s.append(float(e.kernel_ms))
    theta_k = Th[:, cols_t].contiguous()
    tf = ["log"] * k
    names = cap.COV_STATUS_NAMES

    def measure(th_k, f, n_data):
        nd = torch.full((th_k.shape[0],), n_data, dtype=torch.int32, device="cuda")
        ours = lambda: pkg.fit_covariance(p, th_k, f.cost, f.grad, f.JtJ, n_data=nd, transform=tf, keys=keys)

        def torch_composition():
            s = th_k[:, :, None] * th_k[:, None, :]
            Hs = f.JtJ * s
            r = torch.sqrt(torch.diagonal(Hs, dim1=1, dim2=2))
            rr = r[:, :, None] * r[:, None, :]
            C = Hs / rr
            L, _ = torch.linalg.cholesky_ex(C)
            P = torch.cholesky_inverse(L)
            d = torch.sqrt(torch.diagonal(P, dim1=1, dim2=2))
            sigma2 = 2.0 * f.cost / (n_data - k)
            cov = s * (P * sigma2[:, None, None] / rr)
            ev, V = torch.linalg.eigh(C)
            return sigma2, cov, torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)), P / (d[:, :, None] * d[:, None, :]), ev, V, 1.0 / torch.sqrt(ev[:, 0])

        cv, tc = ours(), torch_composition(); torch.cuda.synchronize()           # warm-up of both
        ms_k, ms_t = [], []
        for _ in range(a.reps):
            ms_k.append(timed(ours)[0])
            ms_t.append(timed(torch_composition)[0])
        st, coll, ev = cv.status.cpu().numpy(), cv.collinearity.cpu().numpy(), cv.eval.cpu().numpy()
        plain = st == 0
        q = lambda x: {"p10": float(np.nanpercentile(x, 10)), "median": float(np.nanmedian(x)), "p90": float(np.nanpercentile(x, 90))}
        d_ev = float(np.abs(ev[plain] - tc[4].cpu().numpy()[plain]).max()) if plain.any() else None
        return {"problems": int(th_k.shape[0]), "n_data": n_data, "plh_fit_cov": spread(ms_k), "torch_composition": spread(ms_t), "ours_over_torch_composition": float(np.median(ms_k) / np.median(ms_t)),
                "ours_over_sens_integration": float(np.median(ms_k) / np.median(ms_s)), "torch_composition_over_sens_integration": float(np.median(ms_t) / np.median(ms_s)),
                "status_counts": {nm: int(((st & b) != 0).sum()) for b, nm in names.items()}, "status_0": int(plain.sum()), "collinearity": q(coll[np.isfinite(coll)]),
                "max_abs_eval_difference_to_eigh_status_0": d_ev}

    labels = np.repeat(np.arange(n // 4), 4)
    gf = fit.by_group(labels)
    first = torch.from_numpy(np.arange(0, n, 4)).cuda()
    rec = {"cells": n, "n_q": n_q, "keys": keys, "transform": "log", "sens_integration": spread(ms_s),
           "fit_cov": {"%d_problems" % n: measure(theta_k, fit, n_q), "%d_groups_of_4" % (n // 4): measure(theta_k[first].contiguous(), gf, 4 * n_q)},
           "build_info": p._lib.plh_build_info().decode()}
    if a.c2_line:                                                               # the integrator of the same binary on the same box
        b = json.loads([line for line in open(a.c2_line) if line.startswith('{"metric"')][-1])
        rec["bench_c2_same_box"] = dict({x: b[x] for x in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")}, kernel_ms_avg=b["roofline"]["kernel_ms_avg"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
