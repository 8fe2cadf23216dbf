"""plh_predict / EnsembleSolution.predict / EnsembleFitResult.predict on the GPU: device pointers on a stream of the caller's against host pointers (the same kernels: the
same bits), both against the scipy-built yardstick within the bounds of tests/predict_cases.py; the chunked workspace; a real ensemble in HBM from the fit to the band, tied
together by the hat-matrix identity; the bands of a grouped fit."""
import numpy as np
import pytest

import parity
import predict_cases as pc
import resample_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem(pkg):
    return pc.make_problem(pkg, "main")


def test_device_pointers_on_a_stream_equal_host_pointers(hip_model, pkg, problem):
    import torch
    pb, cap, K = problem, pkg._capi, 8
    k = pb.k
    stream = torch.cuda.Stream()
    for ex in (0, 1):
        code, (host,), hstat = pc.call(pkg, hip_model, k, K, ex, cov=pb.cov[K])
        assert code == 0, hip_model._lib.plh_last_error()
        code, (dev,), dstat = pc.call(pkg, hip_model, k, K, ex, cov=pb.cov[K], kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
        assert code == 0, hip_model._lib.plh_last_error()
        assert pc.same_bits(host, dev) and (hstat == 0).all() and (dstat == 0).all()
        for c in range(k.n):
            pc.check_cell(pb, K, ex, c, pc.cell_of(dev, c), pb.cov[K][c], "device pointers")
    # grouped, three channels: the offsets' device copy, and the kernel argument at its widest
    G = pb.cov[K][[2, 0]]
    kw = dict(cov=G, group_off=[0, 2, 3], n_groups=2)
    code, (host,), _ = pc.call(pkg, hip_model, k, K, 0, **kw)
    assert code == 0, hip_model._lib.plh_last_error()
    for _ in range(2):                                                                     # (the second call finds the offsets on the device)
        code, (dev,), _ = pc.call(pkg, hip_model, k, K, 0, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda", **kw)
        assert code == 0 and pc.same_bits(host, dev)
    for c, g in ((0, 0), (1, 0), (2, 1)):
        pc.check_cell(pb, K, 0, c, pc.cell_of(dev, c), G[g], "grouped, device pointers")
    K3 = 3
    code, h3, _ = pc.call(pkg, hip_model, k, K3, 0, cov=pb.cov[K3], chans=(0, 4, 5))
    code2, d3, _ = pc.call(pkg, hip_model, k, K3, 0, cov=pb.cov[K3], chans=(0, 4, 5), kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and code2 == 0 and all(pc.same_bits(a, b) for a, b in zip(h3, d3))
    for i, f in enumerate((0, 4, 5)):
        for c in range(k.n):
            pc.check_cell(pb, K3, 0, c, pc.cell_of(d3[i], c), pb.cov[K3][c], "three channels, column %d" % f, first=f)


def test_chunked_workspace_gives_the_same_bits(hip_model, pkg, monkeypatch):
    """the nine-cell case of test_gpu_lsq.py::test_chunked_workspace_gives_the_same_bits"""
    import torch
    cap, K = pkg._capi, 8
    pts = ((5, 9), (1, 2), (70, 3), (4, 4), (2, 30), (7, 100), (3, 3), (64, 64), (2, 2))
    k = rc.make_case(pkg, cell_points=pts, width=1 + K, seed=5)
    A = np.random.default_rng(1).standard_normal((k.n, K, 2 * K))
    cov = A @ A.transpose(0, 2, 1)                                                         # (any positive definite matrices: the bits are compared, not the values)
    stream = torch.cuda.Stream()
    code, (whole,), status = pc.call(pkg, hip_model, k, K, 0, cov=cov, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    fin = ~np.isnan(k.tq)
    assert code == 0 and (status == 0).all() and all(np.isfinite(whole[nm][..., fin]).all() for nm in pc.OUTS) and (whole["var"][:, fin] > 0).all()
    monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(2 * 8 * k.max_pts * (1 + K) + 8192))   # two cells' slopes: five chunks
    code, (got,), _ = pc.call(pkg, hip_model, k, K, 0, cov=cov, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and pc.same_bits(got, whole)
    code, (got,), _ = pc.call(pkg, hip_model, k, K, 0, cov=cov)                            # and through host pointers
    assert code == 0 and pc.same_bits(got, whole)


def end_to_end(p, pkg, device):
    """simulate_ensemble(sens=keys) -> ens.lsq -> fit_covariance (absolute sigma) -> ens.predict at the same times; device=True: everything in HBM on a stream of the
    caller's.  The checks are those of test_ensemble_in_hbm_from_the_fit_to_the_band"""
    n, keys = 8, ["D_sp", "k_p"]
    K = len(keys)
    rng = np.random.default_rng(2)
    scale = 2.0 ** (2 * rng.random((n, 2)) - 1)
    Th = pkg.theta_matrix(p, n, {"D_sp": p.θ["D_sp"] * scale[:, 0], "k_p": p.θ["k_p"] * scale[:, 1]})
    cols = [p.θ_keys.index(kn) for kn in keys]
    proto = [{"I": 2.0, "tf": 1000.0, "SOC_max": 0.2}, {"I": -1.0, "tf": 100.0}]
    if device:
        import torch
        stream = torch.cuda.Stream()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        host = lambda a: a.cpu().numpy()
        sync = torch.cuda.synchronize
        ens = pkg.simulate_ensemble(p, up(Th), proto, SOC=0.1, device=True, sens=keys, stream=stream.cuda_stream)
        st = stream.cuda_stream
    else:
        up = host = lambda a: np.asarray(a)
        sync = lambda: None
        ens = pkg.simulate_ensemble(p, Th, proto, SOC=0.1, sens=keys)
        st = None
    sync()
    n_pts, t = host(ens.n_pts), host(ens.t)
    last = np.array([t[i, n_pts[i] - 1] for i in range(n)])
    tq = np.concatenate([rng.uniform(0.0, last.min(), 40), [t[0, 5], ens.run_info[0, 0]["t_end"]]])          # inside the shortest cell's span, a saved time and a join
    tq = tq[rng.permutation(len(tq))]
    data = ens(tq, fields="V").V[0]
    wh = 0.5 + rng.random(len(tq))
    fit = ens.lsq(tq, data, weights=up(wh))
    cv = pkg.fit_covariance(p, up(Th[:, cols]), fit.cost, fit.grad, fit.JtJ, n_data=None, stream=st, keys=keys)      # absolute sigma: sigma2 = 1
    pr = ens.predict(tq, cv)
    if device:
        for a, shape in ((pr.V, (n, len(tq))), (pr.dV_dtheta, (n, K, len(tq))), (pr.V_var, (n, len(tq))), (pr.V_sd, (n, len(tq))), (pr.status, (n,))):
            assert isinstance(a, torch.Tensor) and a.is_cuda and tuple(a.shape) == shape
    assert pr.keys == keys and pr.channels == ["V"] and pr.I is None and pr.T_avg is None
    sync()
    assert (host(pr.status) == 0).all() and (host(cv.status) == 0).all()
    pred, dpred, var, sd, cov, JtJ = (host(a) for a in (pr.V, pr.dV_dtheta, pr.V_var, pr.V_sd, cv.cov, fit.JtJ))
    assert (np.abs(sd - np.sqrt(np.maximum(var, 0.0))) <= 2.0 ** -52 * sd).all()
    # the scipy-built reference from host copies of what the ensemble holds
    k = rc.Case()
    k.n, k.n_runs, k.max_pts, k.width, k.tq = n, 2, t.shape[1], 1 + K, tq
    k.t, k.n_pts, k.run_info = t, n_pts, ens.run_info
    k.src = np.concatenate([host(ens.V)[:, :, None], host(ens.dV_dtheta).transpose(0, 2, 1)], axis=2)
    k.runs = [[(int(sum(ens.run_info[c, :r]["iterations"])), int(ens.run_info[c, r]["iterations"])) for r in range(2)] for c in range(n)]
    pb = pc.Problem()
    pb.k, pb.S = k, {0: rc.fitpack_reference(k, 0)}
    eps = 2.0 ** -52
    for c in range(n):
        pc.check_cell(pb, K, 0, c, dict(pred=pred[c], dpred=dpred[c], var=var[c]), cov[c], "ens.predict")
        # the hat-matrix identity: sum_q w_q^2 var_q = trace(cov JtJ) = k.  It ties plh_lsq_multi's JtJ, plh_fit_cov's covariance and plh_predict's var together.
        # Tolerance: the relative error of P = C^-1 (cov_cases: 64 k eps cond2(C), C the normalised information matrix) on a trace of k, and the bound of every var_q
        r = np.sqrt(np.diag(JtJ[c]))
        cond = float(np.linalg.cond(JtJ[c] / np.outer(r, r)))
        ref = pc.reference(pb.S[0][c], K, cov[c])
        tol = K * 64.0 * K * eps * cond + float((wh ** 2 * pc.bounds(k, c, K, ref, cov[c])["var"]).sum())
        hat = float((wh ** 2 * var[c]).sum())
        s = pb.S[0][c][:, 1:1 + K].T.astype(np.longdouble)
        hat_ref = float(((wh.astype(np.longdouble) ** 2) * (s * (cov[c].astype(np.longdouble) @ s)).sum(axis=0)).sum())
        print("cell %d: sum w^2 var = k + %.3e (longdouble from host copies: k + %.3e), tolerance %.3e, cond2(C) %.3g, sd of V %.3g .. %.3g V"
              % (c, hat - K, hat_ref - K, tol, cond, sd[c].min(), sd[c].max()))
        assert abs(hat_ref - K) <= 0.1 * tol, (c, hat_ref - K, tol)
        assert abs(hat - K) <= tol, (c, hat - K, tol)
    return pr


def test_ensemble_in_hbm_from_the_fit_to_the_band(hip_model, pkg):
    """8 cells, keys D_sp and k_p, the two-run protocol of test_gpu_lsq.py::test_ensemble_in_hbm_against_the_scipy_reference: pred, dpred and var against scipy on host
    copies within the bounds, and sum_q w_q^2 var_q = k per cell"""
    end_to_end(hip_model, pkg, True)


def test_bands_of_a_grouped_fit(hip_model, pkg):
    """the grouped fit of test_fit_groups.py::test_grouped_fit_recovers_parameters_in_hbm (8 groups of three C-rates): res.predict(t) under both weight conventions
    (absolute_sigma False / True) gives finite bands for every member, and the members of a group are banded with the group's covariance.  The z-scores of held-out times
    against the curve at the true parameters are printed, not asserted: a statistic of one seed"""
    import torch
    p, ng, m, keys = hip_model, 8, 3, ["D_sp", "k_p"]
    n, K = ng * m, 2
    cols = [p.θ_keys.index(kn) for kn in keys]
    groups = np.repeat(np.arange(ng), m)
    proto = [{"I": np.tile([-0.5, -1.0, -2.0], ng), "tf": 300.0}]
    o = pkg.Opts(); o.reltol, o.abstol, o.maxiters = parity.TIGHT["reltol"], parity.TIGHT["abstol"], 200000
    t = np.linspace(15.0, 285.0, 16)
    t_out = 0.5 * (t[1:] + t[:-1])                                                         # held out: between the fitted times
    truth = pkg.theta_matrix(p, n)
    sV = 1e-3
    rng = np.random.default_rng(6)
    at_truth = pkg.simulate_ensemble(p, truth, proto, SOC=0.9, opts=o)
    V_true, V_out = np.asarray(at_truth(t, fields="V").V), np.asarray(at_truth(t_out, fields="V").V)
    V_data = np.ascontiguousarray(V_true + sV * rng.standard_normal((n, len(t))))
    wV = np.full(len(t), 1.0 / sV)
    Theta0 = truth.copy()
    Theta0[:, cols] *= np.repeat(2.0 ** rng.uniform(-0.5, 0.5, size=(ng, 2)), m, axis=0)
    stream = torch.cuda.Stream()
    res = pkg.fit_ensemble(p, torch.from_numpy(Theta0).cuda(), proto, keys, t, V_data, wV, SOC=0.9, opts=o, transform={kn: "log" for kn in keys}, max_iter=20, device=True,
                           stream=stream.cuda_stream, lm=dict(ftol=1e-10), groups=groups)
    for absolute in (False, True):
        pr = res.predict(t_out, absolute_sigma=absolute)
        cv = res.covariance(absolute)
        stream.synchronize()
        torch.cuda.synchronize()
        for a, shape in ((pr.V, (n, len(t_out))), (pr.dV_dtheta, (n, K, len(t_out))), (pr.V_var, (n, len(t_out))), (pr.V_sd, (n, len(t_out))), (pr.status, (n,))):
            assert isinstance(a, torch.Tensor) and a.is_cuda and tuple(a.shape) == shape
        V, dV, var, sd, cov = (a.cpu().numpy() for a in (pr.V, pr.dV_dtheta, pr.V_var, pr.V_sd, cv.cov))
        assert (pr.status.cpu().numpy() == 0).all() and cov.shape == (ng, K, K)
        assert np.isfinite(V).all() and np.isfinite(dV).all() and np.isfinite(var).all() and (var > 0).all() and (np.abs(sd - np.sqrt(var)) <= 2.0 ** -52 * sd).all()
        # every member's var is s' M s with ITS GROUP's matrix and its own resampled sensitivities: 2 K + 2 roundings, the slack of predict_cases
        for c in range(n):
            M = cov[groups[c]].astype(np.longdouble)
            s = dV[c].astype(np.longdouble)
            want = (s * (M @ s)).sum(axis=0)
            A = np.einsum("iq,ij,jq->q", np.abs(s), np.abs(M), np.abs(s))
            assert (np.abs(var[c] - want.astype(np.float64)) <= (64.0 * K * 2.0 ** -52 * A).astype(np.float64)).all(), c
        z = (V - V_out) / sd
        print("grouped fit, absolute_sigma %s: sd of V %.3g .. %.3g V at the held-out times; z against the curve at the truth: mean %.3f, rms %.3f, max |z| %.3f; |z| <= 2 in %d of %d"
              % (absolute, sd.min(), sd.max(), z.mean(), np.sqrt((z ** 2).mean()), np.abs(z).max(), int((np.abs(z) <= 2).sum()), z.size))
