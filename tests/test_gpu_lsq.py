"""plh_lsq / EnsembleSolution.lsq on the GPU: device pointers on a stream of the caller's against host pointers (the same kernels: the same bits), both against the scipy-built
yardstick within the bounds of tests/lsq_cases.py; a real ensemble in HBM with sensitivities; the chunked workspace."""
import numpy as np
import pytest

import lsq_cases as lc
import resample_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem(pkg):
    return lc.make_problem(pkg, "main")


@pytest.mark.parametrize("K", (8, 0))
def test_device_pointers_on_a_stream_equal_host_pointers(hip_model, pkg, problem, K):
    import torch
    pb, cap = problem, pkg._capi
    k = pb.k
    stream = torch.cuda.Stream()
    for ex in (0, 1):
        code, host = lc.call(pkg, hip_model, k, K, pb.Y, pb.W[ex], 1, ex)
        assert code == 0, hip_model._lib.plh_last_error()
        code, dev = lc.call(pkg, hip_model, k, K, pb.Y, pb.W[ex], 1, ex, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
        assert code == 0, hip_model._lib.plh_last_error()
        assert lc.same_bits(host, dev) and (host["status"] == 0).all() and (dev["status"] == 0).all()
        if K:
            assert np.array_equal(dev["JtJ"], dev["JtJ"].transpose(0, 2, 1))
        for c in range(k.n):
            lc.check_cell(pb, K, ex, c, lc.cell_of(dev, c), pb.Y[c], pb.W[ex][c], "device pointers")
            code, one = lc.call(pkg, hip_model, k, K, pb.Y[c], pb.W[ex][c], 0, ex, cells=[c], kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
            assert code == 0 and lc.same_bits(lc.cell_of(one, 0), lc.cell_of(dev, c))                      # shared data, cell by cell


def test_ensemble_in_hbm_against_the_scipy_reference(hip_model, pkg):
    import torch
    p, n = hip_model, 8
    rng = np.random.default_rng(2)
    scale = 2.0 ** (2 * rng.random((n, 2)) - 1)
    Th = pkg.theta_matrix(p, n, {"D_sp": p.θ["D_sp"] * scale[:, 0], "k_p": p.θ["k_p"] * scale[:, 1]})
    proto = [{"I": 2.0, "tf": 1000.0, "SOC_max": 0.2}, {"I": -1.0, "tf": 100.0}]
    keys = ["D_sp", "k_p"]
    stream = torch.cuda.Stream()
    ens = pkg.simulate_ensemble(p, torch.from_numpy(Th).cuda(), proto, SOC=0.1, device=True, sens=keys, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    n_pts, t = ens.n_pts.cpu().numpy(), ens.t.cpu().numpy()
    last = np.array([t[i, n_pts[i] - 1] for i in range(n)])
    tq = np.concatenate([rng.uniform(0.0, last.min(), 40), [t[0, 5], ens.run_info[0, 0]["t_end"]]])          # inside the shortest cell's span, a saved time and a join
    tq = tq[rng.permutation(len(tq))]
    data = ens(tq, fields="V").V[0]                                                                        # (a CUDA tensor: stays in HBM)
    w = torch.from_numpy(0.5 + rng.random(len(tq))).cuda()
    fit = ens.lsq(tq, data, weights=w, resid=True)
    for a, shape in ((fit.cost, (n,)), (fit.grad, (n, 2)), (fit.JtJ, (n, 2, 2)), (fit.resid, (n, len(tq))), (fit.status, (n,))):
        assert isinstance(a, torch.Tensor) and a.is_cuda and tuple(a.shape) == shape
    assert fit.keys == keys
    torch.cuda.synchronize()
    assert (fit.status.cpu().numpy() == 0).all()
    # the scipy-built reference from host copies of what the ensemble holds
    k = rc.Case()
    k.n, k.n_runs, k.max_pts, k.width, k.tq = n, 2, t.shape[1], 3, tq
    k.t, k.n_pts, k.run_info = t, n_pts, ens.run_info
    k.src = np.concatenate([ens.V.cpu().numpy()[:, :, None], ens.dV_dtheta.cpu().numpy().transpose(0, 2, 1)], axis=2)
    k.runs = [[(int(sum(ens.run_info[c, :r]["iterations"])), int(ens.run_info[c, r]["iterations"])) for r in range(2)] for c in range(n)]
    pb = lc.Problem()
    pb.k, pb.S = k, {0: rc.fitpack_reference(k, 0)}
    y, wh = data.cpu().numpy(), w.cpu().numpy()
    cost, grad, JtJ, resid = (a.cpu().numpy() for a in (fit.cost, fit.grad, fit.JtJ, fit.resid))
    for c in range(n):
        ref = lc.reference(pb.S[0][c], y, wh)
        lc.check_cell(pb, 2, 0, c, dict(cost=cost[c], grad=grad[c], JtJ=JtJ[c], resid=resid[c]), y, wh, "ens.lsq in HBM")
        if c == 0:                                                                                         # its own curve: the misfit is rounding
            bnd = lc.bounds(k, 0, 2, ref, wh)
            print("cell 0 against its own curve: cost %.3e (bound %.3e)" % (cost[0], bnd["cost"]))
            assert cost[0] <= bnd["cost"]
    assert cost[1:].min() > 1e3 * cost[0]


def test_chunked_workspace_gives_the_same_bits(hip_model, pkg, monkeypatch):
    import torch
    cap, K = pkg._capi, 8
    pts = ((5, 9), (1, 2), (70, 3), (4, 4), (2, 30), (7, 100), (3, 3), (64, 64), (2, 2))
    k = rc.make_case(pkg, cell_points=pts, width=1 + K, seed=5)
    rng = np.random.default_rng(1)
    Y, W = 4.0 + rng.random((k.n, len(k.tq))), np.where(np.isnan(k.tq), 0.0, 0.5 + rng.random((k.n, len(k.tq))))
    stream = torch.cuda.Stream()
    code, whole = lc.call(pkg, hip_model, k, K, Y, W, 1, 0, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and (whole["status"] == 0).all() and np.isfinite(whole["JtJ"]).all()
    monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(2 * 8 * k.max_pts * (1 + K) + 8192))                   # two cells' slopes: five chunks
    code, got = lc.call(pkg, hip_model, k, K, Y, W, 1, 0, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and lc.same_bits(got, whole)
    code, got = lc.call(pkg, hip_model, k, K, Y, W, 1, 0)                                                  # and through host pointers
    assert code == 0 and lc.same_bits(got, whole)
