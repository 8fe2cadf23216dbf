"""ens(t) on the GPU, measured (reported, not gated: bench.py is the yardstick of the integrator and does not know this call).

  python tools/resample_bench.py [--out profiles/resample.json] [--points 200] [--reps 7]

Two jobs, both on a 200-point grid shared by all cells, timed with HIP events around ens(tq) on the launch stream (median of --reps after one warm-up):
  c4_c_e     the C4 shard (8192 jittered cells, 1C discharge) saved with sections=("c_e",): V, I, SOC and the 30 columns of Y_sel
  all_1024   1024 of those cells saved with outputs="all": V, I, SOC and the 301 columns of Y_all
Per job: bytes that must move (the saved points of t and of every field once in, the result once out), the share of the HBM peak that is at the measured time, the
traffic the three kernels actually ask for (slopes written twice and read once, two rows of values and slopes per query), the same job through ens[i](tq) -- scipy splrep
per state column on the host -- timed on 16 cells and scaled to the ensemble, and the ratio to the integrate kernel's own time.  Merges "gpu" into the JSON at --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def job(pkg, p, name, n, n_q, reps, **save):
    import torch
    cfg = pkg.configs.c4(p, n)
    ens = pkg.simulate_ensemble(p, torch.from_numpy(cfg["theta"]).cuda(), cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], **save)
    torch.cuda.synchronize()
    n_pts = ens.n_pts.cpu().numpy().astype(np.int64)
    t_end = float(ens.run_info["t_end"][:, -1].max())
    tq = np.linspace(0.0, t_end, n_q)
    fields = [f for f in ("V", "I", "SOC", "Y_all", "Y_sel") if getattr(ens, f) is not None]
    widths = {f: (1 if getattr(ens, f).ndim == 2 else getattr(ens, f).shape[2]) for f in fields}
    res = ens(tq)                                          # warm-up: workspace, the query grid's device copy
    torch.cuda.synchronize()
    ok = int((res.status == 0).sum())
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = ens(tq)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms_med = float(np.median(ms))
    pts, W = int(n_pts.sum()), sum(widths.values())
    must = 8 * (len(fields) * pts + pts * W + n * n_q * W)                         # t per call + the saved points once + the result once
    asked = must + 8 * (3 * pts * W + 4 * n * n_q * W)                              # + slopes (2 writes, 1 read) + per query two rows of values and two of slopes
    t0 = time.perf_counter()
    for i in range(16):
        ens[i](tq)
    host_s = (time.perf_counter() - t0) / 16 * n
    return {"job": name, "cells": n, "cells_resampled": ok, "n_q": n_q, "fields": widths, "saved_points": pts, "ms_median": ms_med, "ms_all": [float(x) for x in ms],
            "bytes_must_move": must, "hbm_share_of_must_move": must / (ms_med * 1e-3) / HBM_PEAK, "bytes_kernels_ask_for": asked,
            "hbm_share_of_asked": asked / (ms_med * 1e-3) / HBM_PEAK, "host_route_s_scaled_from_16_cells": host_s, "speedup_vs_host_route": host_s / (ms_med * 1e-3),
            "integrate_kernel_ms": float(ens.kernel_ms), "ratio_to_integrate_kernel": ms_med / float(ens.kernel_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "resample_bench.py needs a GPU"
    torch.cuda.init()                                      # (torch's runtime first, as in bench.py and smoke(): the library then joins the device torch opened)
    import pkgload
    pkg = pkgload.load()
    p = pkg.petlion(pkg.LCO)
    jobs = [job(pkg, p, "c4_c_e", 8192, a.points, a.reps, sections=("c_e",)), job(pkg, p, "all_1024", 1024, a.points, a.reps, outputs="all")]
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec["gpu"] = {"hbm_peak_bytes_per_s": HBM_PEAK, "jobs": jobs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec["gpu"]))


if __name__ == "__main__":
    main()
