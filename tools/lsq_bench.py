"""ens.lsq on the GPU, measured (reported, not gated: bench.py is the yardstick of the integrator and does not know this call).

  python tools/lsq_bench.py [--out profiles/lsq.json] [--cells 8192] [--points 200] [--reps 7] [--fd-cells 16]

Shape: the C4 shard (8192 jittered cells, 1C discharge) integrated with sens = the seven sweep parameters, device=True, and 200 measurement times shared by all cells.
  fused        ens.lsq(tq, data, weights): cost [n], grad [n, 7], JtJ [n, 7, 7] in HBM (plh_lsq)
  composition  what the API offered for the same result before plh_lsq, everything in HBM: ens(tq, fields="V"), plh_resample on dV_dtheta.transpose(1, 2).contiguous() with
               width 7, and the torch reductions
Both timed with HIP events in the same process, alternating, median of --reps after one warm-up each, with their run-to-run spread; the two results are compared.  Also
recorded: the ratio to the sensitivity kernel's own time, the bytes that would otherwise cross to the host, and one finite-difference check made at reltol = abstol = 1e-8 on
the first --fd-cells cells (measurement times up to the end of the shortest trajectory, and up to 0.9 of it): grad against central differences of cost over two extra plain
runs per parameter and step (relative steps 1e-2, 1e-3, 1e-4; the yardstick is DESIGN.md 3's 7e-5 for
dV/dtheta against differenced runs).  Writes the JSON at --out.

  python tools/lsq_bench.py --channels [--out profiles/lsq_channels.json]

The `channels` record, same shard and times: (a) one fused V + I call (plh_lsq_multi, two channels) against two single-channel calls plus the torch additions of their cost,
grad and JtJ, alternating in one process, HIP events, median of --reps after one warm-up, and the difference of the two results; (b) the sensitivity kernel's own time
(plh_last_kernel_ms) with every channel of the model requested against dV/dtheta only, the same binary, alternating --reps times.

  python tools/lsq_bench.py --predict [--out profiles/predict.json]

The `predict` record, same shard and times: plh_predict with all three outputs of the voltage channel (pred, dpred, var; preallocated outputs, device pointers) against
plh_lsq_multi on the same arrays (ens.lsq: the same sweeps, sums instead of stores), alternating in one process, HIP events around --inner back-to-back calls each, median
of --reps after a warm-up, with the spread; ens.predict (the front end: allocations and the square root for sd included) the same way; and the sensitivity kernel's own
time of the integration that feeds them."""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [float(x) for x in ms]}


def measure(pkg, p, n, n_q, reps):
    import torch
    cap = pkg._capi
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    cfg = pkg.configs.c4(p, n)
    ens = pkg.simulate_ensemble(p, torch.from_numpy(cfg["theta"]).cuda(), cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys)
    torch.cuda.synchronize()
    sens_ms = float(ens.kernel_ms)
    t_end = float(ens.run_info["t_end"][:, -1].min())
    tq = np.linspace(0.0, t_end, n_q)
    rng = np.random.default_rng(0)
    data = ens(tq, fields="V").V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()          # cell 0's curve plus 2 mV of noise
    w = torch.from_numpy(0.5 + rng.random(n_q)).cuda()
    ns, mp = len(keys), ens.t.shape[1]
    lib, h = p._lib, p._h

    def fused():
        f = ens.lsq(tq, data, weights=w)
        return f.cost, f.grad, f.JtJ

    def composition():
        S_V = ens(tq, fields="V").V                                                                    # [n, n_q]
        src = ens.dV_dtheta.transpose(1, 2).contiguous()                                               # [n, max_pts, 7]: the layout plh_resample takes
        S = torch.empty(n, n_q, ns, dtype=torch.float64, device=src.device)
        cap.check(lib, lib.plh_resample(h, n, len(ens.run_names), mp, ens.t.data_ptr(), ens.n_pts.data_ptr(), ens._run_info_raw.data_ptr(), ns, src.data_ptr(), n_q, tq.ctypes.data, 0,
                                        S.data_ptr(), None, cap.PLH_DEVICE, None), "plh_resample")
        r = w * (S_V - data)
        J = w[None, :, None] * S
        return 0.5 * (r * r).sum(dim=1), torch.einsum("nqk,nq->nk", J, r), torch.einsum("nqk,nql->nkl", J, J)

    a, b = fused(), composition()                                                                      # warm-up of both: workspaces, the query grid's device copy, torch's kernels
    torch.cuda.synchronize()
    agree = {nm: float(((x - y).abs().max() / y.abs().max()).cpu()) for nm, x, y in zip(("cost", "grad", "JtJ"), a, b)}
    ms_f, ms_c = [], []
    for _ in range(reps):                                                                              # alternating: both see the same machine
        ms_f.append(timed(fused)[0])
        ms_c.append(timed(composition)[0])
    rec = {"cells": n, "n_q": n_q, "sens_keys": keys, "max_pts": mp, "cells_ok": int((ens.lsq(tq, data).status == 0).sum()),
           "fused": spread(ms_f), "composition": spread(ms_c), "fused_over_composition": float(np.median(ms_f) / np.median(ms_c)),
           "max_abs_difference_over_max_abs": agree,
           "sens_kernel_ms": sens_ms, "fused_over_sens_kernel": float(np.median(ms_f)) / sens_ms,
           "bytes_to_host_without_it": 8 * n * mp * (2 + ns), "bytes_to_host_with_it": 8 * n * (1 + ns + ns * ns)}
    return rec, keys


def measure_channels(pkg, p, n, n_q, reps):
    import torch
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    cfg = pkg.configs.c4(p, n)
    Th = torch.from_numpy(cfg["theta"]).cuda()
    run = lambda outs: pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys, sens_outputs=outs)
    chans = ("V", "I", "T_avg") if p.temperature else ("V", "I")
    ens = run(chans)                                                                                   # warm-up of the kernel, and the ensemble the lsq calls work on
    torch.cuda.synchronize()
    run(("V",)); torch.cuda.synchronize()
    ms_all, ms_v = [], []
    for _ in range(reps):                                                                              # (b) alternating: both see the same machine
        e = run(chans); torch.cuda.synchronize(); ms_all.append(float(e.kernel_ms))
        e = run(("V",)); torch.cuda.synchronize(); ms_v.append(float(e.kernel_ms))
    t_end = float(ens.run_info["t_end"][:, -1].min())
    tq = np.linspace(0.0, t_end, n_q)
    rng = np.random.default_rng(0)
    res = ens(tq, fields=("V", "I"))
    dV = res.V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()
    dI = res.I[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()
    wV, wI = torch.from_numpy(0.5 + rng.random(n_q)).cuda(), torch.from_numpy(0.5 + rng.random(n_q)).cuda()

    def fused():
        f = ens.lsq(tq, dV, weights=wV, I_data=dI, I_weights=wI)
        return f.cost, f.grad, f.JtJ

    def separate():
        a, b = ens.lsq(tq, dV, weights=wV), ens.lsq(tq, I_data=dI, I_weights=wI)
        return a.cost + b.cost, a.grad + b.grad, a.JtJ + b.JtJ

    a, b = fused(), separate()
    torch.cuda.synchronize()
    agree = {nm: float(((x - y).abs().max() / y.abs().max()).cpu()) for nm, x, y in zip(("cost", "grad", "JtJ"), a, b)}
    ms_f, ms_s = [], []
    for _ in range(reps):
        ms_f.append(timed(fused)[0])
        ms_s.append(timed(separate)[0])
    return {"cells": n, "n_q": n_q, "sens_keys": keys, "max_pts": int(ens.t.shape[1]),
            "lsq": {"channels": ["V", "I"], "fused": spread(ms_f), "separate_calls_plus_torch_additions": spread(ms_s), "fused_over_separate": float(np.median(ms_f) / np.median(ms_s)),
                    "max_abs_difference_over_max_abs": agree},
            "sens_kernel": {"channels_all": list(chans), "all_channels": spread(ms_all), "dV_only": spread(ms_v), "all_over_dV_only": float(np.median(ms_all) / np.median(ms_v)),
                            "against_the_parent_build": "not measured: no build of the parent commit on the box"}}


def measure_predict(pkg, p, n, n_q, reps, inner):
    import torch
    cap = pkg._capi
    keys = [k for k in pkg.configs.SWEEP_KEYS if k in p.θ_keys]
    cfg = pkg.configs.c4(p, n)
    Th = torch.from_numpy(cfg["theta"]).cuda()
    ens = pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sens=keys)
    torch.cuda.synchronize()
    sens_ms = float(ens.kernel_ms)
    t_end = float(ens.run_info["t_end"][:, -1].min())
    tq = np.linspace(0.0, t_end, n_q)
    rng = np.random.default_rng(0)
    data = ens(tq, fields="V").V[0] + torch.from_numpy(2e-3 * rng.standard_normal(n_q)).cuda()          # cell 0's curve plus 2 mV of noise, weights 1 / sigma
    w = torch.full((n_q,), 1.0 / 2e-3, dtype=torch.float64, device="cuda")
    ns, mp = len(keys), ens.t.shape[1]
    fit = ens.lsq(tq, data, weights=w)
    cols = [p.θ_keys.index(k) for k in keys]
    cv = pkg.fit_covariance(p, Th[:, cols].contiguous(), fit.cost, fit.grad, fit.JtJ, keys=keys)        # absolute sigma
    lib, h = p._lib, p._h
    pred, dpred, var = (torch.empty(*shape, dtype=torch.float64, device="cuda") for shape in ((n, n_q), (n, ns, n_q), (n, n_q)))
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    ch = (cap.PredictChannel * 1)(cap.PredictChannel(ens.V.data_ptr(), ens.dV_dtheta.data_ptr(), pred.data_ptr(), dpred.data_ptr(), var.data_ptr()))

    def raw():
        cap.check(lib, lib.plh_predict(h, n, len(ens.run_names), mp, ens.t.data_ptr(), ens.n_pts.data_ptr(), ens._run_info_raw.data_ptr(), 1, ch, ns, n_q, tq.ctypes.data, 0,
                                       cv.cov.data_ptr(), 0, None, status.data_ptr(), cap.PLH_DEVICE, None), "plh_predict")

    routes = {"plh_predict": raw, "ens_predict": lambda: ens.predict(tq, cv), "ens_lsq": lambda: ens.lsq(tq, data, weights=w)}
    for fn in routes.values():                                                                         # warm-up: workspaces, the query grid's device copy, torch's kernels
        fn()
    torch.cuda.synchronize()
    front = ens.predict(tq, cv)
    torch.cuda.synchronize()
    same = bool(torch.equal(front.V, pred) and torch.equal(front.dV_dtheta, dpred) and torch.equal(torch.nan_to_num(front.V_var), torch.nan_to_num(var)))
    ms = {nm: [] for nm in routes}
    for _ in range(reps):                                                                              # alternating: all see the same machine
        for nm, fn in routes.items():
            ms[nm].append(timed(lambda: [fn() for _ in range(inner)])[0] / inner)
    ok = (status == 0) & (cv.status == 0)
    med = {nm: float(np.median(v)) for nm, v in ms.items()}
    return {"cells": n, "n_q": n_q, "sens_keys": keys, "max_pts": int(mp), "calls_per_timed_window": inner, "cells_with_a_band": int(ok.sum()),
            "front_end_has_the_raw_calls_bits": same, "sd_of_V_median_over_cells_and_times": float(torch.nanmedian(front.V_sd).cpu()),
            "plh_predict": spread(ms["plh_predict"]), "ens_predict": spread(ms["ens_predict"]), "ens_lsq": spread(ms["ens_lsq"]),
            "plh_predict_over_ens_lsq": med["plh_predict"] / med["ens_lsq"], "ens_predict_over_ens_lsq": med["ens_predict"] / med["ens_lsq"],
            "sens_kernel_ms": sens_ms, "plh_predict_over_sens_kernel": med["plh_predict"] / sens_ms,
            "bytes_written_per_call": 8 * n * n_q * (2 + ns), "bytes_to_host_without_it": 8 * n * mp * (2 + ns)}


def fd_check(pkg, p, keys, n, n_q, window=1.0, steps=(1e-2, 1e-3, 1e-4)):
    """grad of ens.lsq against central differences of cost: two plain runs per parameter and relative step, everything at reltol = abstol = 1e-8.  A difference quotient has
    its own error -- truncation at a large step (the voltage knee at the end of the discharge is strongly curved in the parameters), the runs' integration error over the
    step at a small one -- so several steps are recorded; the smallest disagreement is an upper bound of the gradient's own error.  window: the measurement times span that
    fraction of the shortest trajectory (1: up to the last saved point, which the integrator places by LINEAR back-interpolation inside its last step when a run ends on a bound;
    that point's error changes with the step pattern of every differenced run)"""
    o = copy.copy(p.opts)
    o.abstol = o.reltol = 1e-8
    cfg = pkg.configs.c4(p, n)
    Th = cfg["theta"]
    run = lambda th, **kw: pkg.simulate_ensemble(p, th, cfg["protocol"], SOC=cfg["SOC"], opts=o, max_points=4096, **kw)
    ens = run(Th, sens=keys)
    tq = np.linspace(0.0, window * float(ens.run_info["t_end"][:, -1].min()), n_q)
    rng = np.random.default_rng(0)
    data = ens(tq, fields="V").V[n - 1] + 2e-3 * rng.standard_normal(n_q)                               # another cell's curve plus 2 mV of noise
    fit = ens.lsq(tq, data)
    scale = np.abs(fit.grad).max(axis=0)                                                               # per parameter, over the cells
    out = {"cells": n, "window": window, "cells_ok": int((fit.status == 0).sum()), "reltol_abstol": 1e-8, "yardstick_dV_dtheta_vs_differenced_runs": 7e-5, "by_relative_step": {}}
    for rel in steps:
        fd = np.zeros_like(fit.grad)
        for j, key in enumerate(keys):
            col = p.θ_keys.index(key)
            c = []
            for s in (+1.0, -1.0):
                T2 = Th.copy()
                T2[:, col] *= 1.0 + s * rel
                c.append(run(T2).lsq(tq, data).cost)
            fd[:, j] = (c[0] - c[1]) / (2.0 * rel * Th[:, col])
        err = np.abs(fd - fit.grad) / scale[None, :]
        out["by_relative_step"]["%g" % rel] = {"max_abs_grad_minus_fd_over_max_abs_grad_per_key": dict(zip(keys, [float(x) for x in err.max(axis=0)])), "worst": float(err.max())}
    out["worst_at_best_step"] = min(v["worst"] for v in out["by_relative_step"].values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--channels", action="store_true", help="the `channels` record (profiles/lsq_channels.json) instead of the plh_lsq one")
    ap.add_argument("--predict", action="store_true", help="the `predict` record (profiles/predict.json): plh_predict against plh_lsq_multi and the sensitivity integration")
    ap.add_argument("--inner", type=int, default=20, help="--predict: calls per timed window")
    ap.add_argument("--cells", type=int, default=8192)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fd-cells", type=int, default=16)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "predict.json" if a.predict else "lsq_channels.json" if a.channels else "lsq.json")
    import torch
    assert torch.cuda.is_available(), "lsq_bench.py needs a GPU"
    torch.cuda.init()                                      # (torch's runtime first, as in bench.py and smoke(): the library then joins the device torch opened)
    import pkgload
    pkg = pkgload.load()
    p = pkg.petlion(pkg.LCO)
    if a.channels or a.predict:
        rec = {"predict": measure_predict(pkg, p, a.cells, a.points, a.reps, a.inner)} if a.predict else {"channels": measure_channels(pkg, p, a.cells, a.points, a.reps)}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rec, open(a.out, "w"), indent=1)
        print(json.dumps(rec))
        return
    rec, keys = measure(pkg, p, a.cells, a.points, a.reps)
    rec = {"gpu": rec}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)             # (the timing survives a failure of the check below)
    rec["gpu"]["finite_difference_check"] = [fd_check(pkg, p, keys, a.fd_cells, a.points, window) for window in (1.0, 0.9)]
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec["gpu"]))


if __name__ == "__main__":
    main()
