"""Shared by tests/test_resample.py (wave emulator) and tests/test_gpu_resample.py: the synthetic ensemble plh_resample is called on, the yardstick
(scipy.interpolate.splrep / splev with s = 0 = FITPACK, the reference's Dierckx, applied run by run with the run-assignment rule of Solution.__call__), a numpy restatement of
the library's algorithm (used ONLY to measure how far that algorithm is from FITPACK in rounding on these very inputs: the tolerance is 100 x that figure), and the raw call.

Tolerance.  In exact arithmetic the not-a-knot cubic in slope form and FITPACK's B-spline for k = 3, s = 0 are the same function; so are the parabola / line of the short
runs.  RESTATEMENT_VS_FITPACK is the largest |restatement - FITPACK| / max|column| over every (cell, column, query) of the case below that lies inside its run's points or
less than one end step outside them, measured on the CPU (test_resample.py::test_restatement_is_as_close_to_fitpack_as_recorded re-measures it on every run and
profiles/resample.json records it); the kernels are held to TOL = 100 x that, the margin being for the device's FMA contraction and the large step ratios of real runs.

Far extrapolation.  The query grid is shared by cells whose runs span 1e-3 s and 1e+3 s, so with extrapolate = 1 a query just behind the longest cell's end lies 1e5 run
lengths outside a short cell's points.  There the value is (distance / step)^3 times the rounding of the data's third differences: two correct implementations differ by
many digits, relative to anything.  Those (cell, query) pairs -- more than one end step outside the points of the run they are assigned to -- are compared only under
extrapolate = 0 (where they clamp to the end point); under extrapolate = 1 they must be finite.  Every other pair is compared under both."""
import ctypes as C

import numpy as np

CELL_POINTS = ((1, 2), (3, 4), (5, 130))      # saved points of (run 0, run 1) per cell: every small-n branch and a long run
MAX_PTS = 140
WIDTHS = (1, 63, 64, 65, 130)                 # around the 64-column tile of one wave
RESTATEMENT_VS_FITPACK = 1.2e-15             # measured 1.11e-15 on the case below (profiles/resample.json); 200 random grids of 4 .. 199 points of the same step pattern gave 5.3e-15
TOL = 100 * RESTATEMENT_VS_FITPACK
E_ARG = -1


def step_grid(rng, n, t0):
    """n times like the integrator's: a first step between 1e-5 and 1e-2 s, then step ratios from {1/4, 1/2, 1, 2}, steps between 1e-6 and 200 s"""
    h = [10 ** rng.uniform(-5, -2)]
    for _ in range(n - 2):
        h.append(min(max(h[-1] * rng.choice([0.25, 0.5, 1, 1, 1, 2, 2]), 1e-6), 200.0))
    return t0 + np.concatenate([[0.0], np.cumsum(h)])[:n]


def values(t, run, width):
    """smooth, different per column, and different per run (the join is a jump: a query assigned to the wrong run shows)"""
    c = np.arange(width)[None, :]
    t = t[:, None]
    return 4.2 - 0.3 * np.sqrt(t / 500.0 + 1e-3) * (1 + 0.01 * c) + 0.05 * np.sin(t / 37.0 + 0.1 * c) + 0.02 * c + 0.5 * run + 0.1 * np.cos(0.3 * c) * np.exp(-t / 90.0)


class Case:
    pass


def make_case(pkg, cell_points=CELL_POINTS, width=max(WIDTHS), seed=11):
    cap = pkg._capi
    rng = np.random.default_rng(seed)
    n, n_runs = len(cell_points), len(cell_points[0])
    k = Case()
    k.n, k.n_runs, k.max_pts, k.width = n, n_runs, MAX_PTS, width
    k.t = np.full((n, MAX_PTS), np.nan)
    k.src = np.full((n, MAX_PTS, width), np.nan)                    # rows past n_pts: NaN -- a read of one shows
    k.n_pts = np.zeros(n, np.int32)
    k.run_info = np.zeros((n, n_runs), cap.RUN_INFO_DTYPE)
    k.runs = []                                                     # per cell: [(first row, points)]
    for c, pts in enumerate(cell_points):
        row, t0, rr = 0, 0.0, []
        for r, m in enumerate(pts):
            tr = step_grid(rng, m, t0)
            k.t[c, row:row + m] = tr
            k.src[c, row:row + m] = values(tr, r, width)
            k.run_info[c, r] = (0 if r else 4, m, tr[-1], 0.0, 0.0, 0.0, 0.0)
            rr.append((row, m))
            row, t0 = row + m, tr[-1]
        k.runs.append(rr)
        k.n_pts[c] = row
    # queries, shared by all cells, unsorted: saved times of every run with >= 2 points (first, last, interior), the joins, before the first point and after the
    # last of every cell (mildly: a quarter of the end step), one NaN, and times spread over the longest cell
    q, k.saved = [], []
    for c in range(n):
        for (row, m) in k.runs[c]:
            if m >= 2:
                pick = sorted(set([row, row + m - 1, row + m // 2, row + 1]))
                q += list(k.t[c, pick])
        q.append(k.run_info[c, 0]["t_end"])
        last = int(k.n_pts[c]) - 1
        q += [k.t[c, 0] - 0.25 * (k.t[c, 1] - k.t[c, 0]), k.t[c, last] + 0.25 * (k.t[c, last] - k.t[c, last - 1])]
    t_long = k.t[n - 1, :int(k.n_pts[n - 1])]
    q += list(rng.uniform(t_long[0], t_long[-1], 40)) + list(10 ** rng.uniform(-6, 0, 12)) + [np.nan]
    q = np.array(q)
    k.tq = np.ascontiguousarray(q[rng.permutation(len(q))])
    return k


def assign_runs(k, c):
    """Solution.__call__'s rule: before the first span -> run 0, else the first run with a <= tq <= b, else the last run (NaN lands there)"""
    which = np.full(k.tq.shape, k.n_runs - 1)
    ends = k.run_info[c]["t_end"]
    spans = [(k.t[c, 0] if r == 0 else ends[r - 1], ends[r]) for r in range(k.n_runs)]
    for q, tv in enumerate(k.tq):
        if tv < spans[0][0]:
            which[q] = 0
            continue
        for r, (a, b) in enumerate(spans):
            if a <= tv <= b:
                which[q] = r
                break
    return which


def mild(k, c):
    """[n_q] bool: the query lies inside the points of its run or less than one end step outside (see the module docstring); NaN queries count as mild"""
    which, ok = assign_runs(k, c), np.ones(k.tq.shape, bool)
    for r, (row, m) in enumerate(k.runs[c]):
        if m < 2:
            continue
        x = k.t[c, row:row + m]
        far = (k.tq < x[0] - (x[1] - x[0])) | (k.tq > x[-1] + (x[-1] - x[-2]))
        ok &= ~((which == r) & far)
    return ok


def fitpack_reference(k, extrapolate):
    """[cell, n_q, width] by scipy, column by column: the yardstick"""
    from scipy.interpolate import splev, splrep
    out = np.full((k.n, len(k.tq), k.width), np.nan)
    good = ~np.isnan(k.tq)
    for c in range(k.n):
        which = assign_runs(k, c)
        for r, (row, m) in enumerate(k.runs[c]):
            sel = (which == r) & good
            if not sel.any():
                continue
            x, y = k.t[c, row:row + m], k.src[c, row:row + m]
            if m == 1:
                out[c, sel] = y[0]
                continue
            for col in range(k.width):
                out[c, sel, col] = splev(k.tq[sel], splrep(x, y[:, col], k=min(3, m - 1), s=0), ext=0 if extrapolate else 3)
    return out


def restatement(k, extrapolate):
    """the algorithm of csrc/plh_resample.h in numpy (all columns of a run at once): slope form, de Boor's not-a-knot rows, Thomas elimination, Hermite evaluation"""
    out = np.full((k.n, len(k.tq), k.width), np.nan)
    good = ~np.isnan(k.tq)
    for c in range(k.n):
        which = assign_runs(k, c)
        for r, (row, n) in enumerate(k.runs[c]):
            sel = (which == r) & good
            if not sel.any():
                continue
            x, y = k.t[c, row:row + n], k.src[c, row:row + n]
            if n == 1:
                out[c, sel] = y[0]
                continue
            tq = k.tq[sel] if extrapolate else np.clip(k.tq[sel], x[0], x[-1])
            h = np.diff(x)
            d = np.diff(y, axis=0) / h[:, None]
            s = np.zeros_like(y)
            if n == 2:
                s[:] = d[0]
            elif n == 3:
                cc = (d[1] - d[0]) / (h[0] + h[1])
                s[0], s[1], s[2] = d[0] - h[0] * cc, d[0] + h[0] * cc, d[1] + h[1] * cc
            else:
                a, b, cu, g = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros_like(y)
                b[0], cu[0] = h[1], h[0] + h[1]
                g[0] = ((3 * h[0] + 2 * h[1]) * h[1] * d[0] + h[0] ** 2 * d[1]) / (h[0] + h[1])
                for i in range(1, n - 1):
                    a[i], b[i], cu[i] = h[i], 2 * (h[i - 1] + h[i]), h[i - 1]
                    g[i] = 3 * (h[i] * d[i - 1] + h[i - 1] * d[i])
                a[n - 1], b[n - 1] = h[n - 2] + h[n - 3], h[n - 3]
                g[n - 1] = ((3 * h[n - 2] + 2 * h[n - 3]) * h[n - 3] * d[n - 2] + h[n - 2] ** 2 * d[n - 3]) / (h[n - 3] + h[n - 2])
                for i in range(1, n):
                    w = a[i] / b[i - 1]
                    b[i] -= w * cu[i - 1]
                    g[i] -= w * g[i - 1]
                s[n - 1] = g[n - 1] / b[n - 1]
                for i in range(n - 2, -1, -1):
                    s[i] = (g[i] - cu[i] * s[i + 1]) / b[i]
            i = np.clip(np.searchsorted(x, tq, side="right") - 1, 0, n - 2)
            u, hi = (tq - x[i])[:, None], h[i][:, None]
            c2 = (3 * d[i] - 2 * s[i] - s[i + 1]) / hi
            c3 = (s[i] + s[i + 1] - 2 * d[i]) / hi ** 2
            out[c, sel] = y[i] + u * (s[i] + u * (c2 + u * c3))
    return out


def scaled_error(k, got, ref, c, rows=None):
    """max over the columns of max|got - ref| / max|column| of cell c (rows: which queries)"""
    scale = np.abs(k.src[c, :int(k.n_pts[c])]).max(axis=0)
    rows = np.ones(len(k.tq), bool) if rows is None else rows
    rows = rows & ~np.isnan(k.tq)
    return float((np.abs(got[c, rows] - ref[c, rows]) / scale[None, :got.shape[2]]).max()) if rows.any() else 0.0


def call(pkg, p, k, extrapolate, width=None, cells=None, want_status=True, kind=None, stream=None, dev=None):
    """plh_resample on the case (the first `width` columns, the listed cells); host pointers, or device tensors made from the same arrays with kind = PLH_DEVICE.
    Returns (rc, dst [cell, n_q, width], status)"""
    cap = pkg._capi
    width = width or k.width
    cells = list(range(k.n)) if cells is None else cells
    t, n_pts, ri = np.ascontiguousarray(k.t[cells]), np.ascontiguousarray(k.n_pts[cells]), np.ascontiguousarray(k.run_info[cells])
    src = np.ascontiguousarray(k.src[cells][:, :, :width])
    n = len(cells)
    dst = np.full((n, len(k.tq), width), -777.0)
    status = np.full(n, -7, np.int32)
    lib = p._lib
    if kind == cap.PLH_DEVICE:
        import torch
        up = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to(dev)
        d = [up(a) for a in (t, n_pts, ri, src, dst, status)]
        rc = lib.plh_resample(p._h, n, k.n_runs, k.max_pts, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), width, d[3].data_ptr(), len(k.tq), k.tq.ctypes.data,
                              extrapolate, d[4].data_ptr(), d[5].data_ptr() if want_status else None, kind, stream)
        torch.cuda.synchronize()
        return rc, d[4].cpu().numpy(), d[5].cpu().numpy()
    rc = lib.plh_resample(p._h, n, k.n_runs, k.max_pts, t.ctypes.data, n_pts.ctypes.data, ri.ctypes.data, width, src.ctypes.data, len(k.tq), k.tq.ctypes.data,
                          extrapolate, dst.ctypes.data, status.ctypes.data if want_status else None, cap.PLH_HOST, None)
    return rc, dst, status
