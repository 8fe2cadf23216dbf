"""plh_lsq_group / plh_group_scatter: the numpy restatement of the definition in include/petlion_hip.h (plain sequential loops), generators of inputs in which the order of
summation shows, the comparison, and the calls on host pointers (tests/test_lsq_group.py, test_fit_groups_analytic.py, test_fit_groups.py).  Nothing here calls the library
except `call_sum` and `call_scatter`."""
import numpy as np

E_ARG = -1
SIZES = [1, 2, 63, 64, 65, 130, 1]          # 326 cells: groups that end before, on and after a wave's width, groups of one at both ends


def offsets(sizes):
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int32)


def labels(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def sum_reference(off, cost, grad, JtJ, status):
    """the header's definition: every entry summed sequentially in ascending cell order, starting from the first member's value.  grad / JtJ / status may be None"""
    ng = len(off) - 1
    k = 0 if grad is None else grad.shape[1]
    g_cost, g_status = np.empty(ng), np.zeros(ng, np.int32)
    g_grad, g_JtJ = (None, None) if grad is None else (np.empty((ng, k)), np.empty((ng, k, k)))
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(ng):
            c0, c1 = int(off[g]), int(off[g + 1])
            acc = cost[c0]
            for c in range(c0 + 1, c1):
                acc = acc + cost[c]
            g_cost[g] = acc
            for i in range(k):
                acc = grad[c0, i]
                for c in range(c0 + 1, c1):
                    acc = acc + grad[c, i]
                g_grad[g, i] = acc
                for j in range(k):
                    acc = JtJ[c0, i, j]
                    for c in range(c0 + 1, c1):
                        acc = acc + JtJ[c, i, j]
                    g_JtJ[g, i, j] = acc
            if status is not None:
                g_status[g] = 1 if (status[c0:c1] != 0).any() else 0
    return g_cost, g_grad, g_JtJ, g_status


def scatter_reference(off, cols, g_theta, theta):
    out = theta.copy()
    for g in range(len(off) - 1):
        for c in range(int(off[g]), int(off[g + 1])):
            for i in cols:
                out[c, i] = g_theta[g, i]
    return out


def make_fits(n, k, seed):
    """per-cell cost [n], grad [n, k], JtJ [n, k, k] (symmetric, as plh_lsq_multi writes it); grad and the off-diagonal of JtJ have mixed signs and magnitudes spread over
    1e-6 .. 1e6, so that sums taken in another order differ in their bits"""
    r = np.random.default_rng(seed)
    mag = lambda *shape: r.choice([-1.0, 1.0], size=shape) * 10.0 ** r.uniform(-6, 6, size=shape)
    cost = 10.0 ** r.uniform(-6, 6, size=n)
    if k == 0:
        return cost, None, None
    grad = mag(n, k)
    A = mag(n, k, k)
    JtJ = np.ascontiguousarray(np.triu(A) + np.transpose(np.triu(A, 1), (0, 2, 1)))
    return cost, np.ascontiguousarray(grad), JtJ


def same_bits_nan(got, ref):
    """NaN where the restatement has NaN, identical bits elsewhere"""
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.where(nan, 0.0, got).tobytes() == np.where(nan, 0.0, ref).tobytes()


def _cap():
    import pkgload
    return pkgload.load()._capi


def call_sum(model, off, cost, grad, JtJ, status, out, n_cells=None, n_groups=None, n_sens=None, null=()):
    """plh_lsq_group on host pointers into out = dict(g_cost, g_grad, g_JtJ, g_status) (entries may be None).  Returns the return code.  null: names passed as NULL"""
    cap = _cap()
    k = 0 if grad is None else grad.shape[1]
    args = dict(group_off=off, cost=cost, grad=grad, JtJ=JtJ, status=status, **out)
    for a in args.values():
        assert a is None or a.flags.c_contiguous
    p = {x: (None if x in null else cap.ptr(a)) for x, a in args.items()}
    return model._lib.plh_lsq_group(model._h, cost.shape[0] if n_cells is None else n_cells, len(off) - 1 if n_groups is None else n_groups, p["group_off"],
                                    k if n_sens is None else n_sens, p["cost"], p["grad"], p["JtJ"], p["status"], p["g_cost"], p["g_grad"], p["g_JtJ"], p["g_status"], cap.PLH_HOST, None)


def call_scatter(model, off, cols, g_theta, theta, n_cells=None, n_groups=None, n_theta=None, n_keys=None, null=()):
    """plh_group_scatter on host pointers, in place on theta.  Returns the return code"""
    cap = _cap()
    ci = np.ascontiguousarray(cols, dtype=np.int32)
    args = dict(group_off=off, cols=ci, g_theta=g_theta, theta=theta)
    p = {x: (None if x in null else cap.ptr(a)) for x, a in args.items()}
    return model._lib.plh_group_scatter(model._h, theta.shape[0] if n_cells is None else n_cells, len(off) - 1 if n_groups is None else n_groups, p["group_off"],
                                        theta.shape[1] if n_theta is None else n_theta, len(ci) if n_keys is None else n_keys, p["cols"], p["g_theta"], p["theta"], cap.PLH_HOST, None)


def sum_outputs(ng, k, fill=None):
    """the four output arrays; fill: a sentinel value (else uninitialised)"""
    mk = (lambda shape, dt=np.float64: np.empty(shape, dt)) if fill is None else (lambda shape, dt=np.float64: np.full(shape, fill, dt))
    return dict(g_cost=mk(ng), g_grad=mk((ng, k)) if k else None, g_JtJ=mk((ng, k, k)) if k else None, g_status=mk(ng, np.int32))
