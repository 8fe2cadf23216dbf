"""plh_resample / EnsembleSolution.__call__ on the GPU: device pointers on a stream of the caller's against host pointers (the same kernels: the same bits), both against
FITPACK with the tolerance of tests/resample_cases.py; an ensemble in HBM against the single-cell host spline; the chunked workspace."""
import numpy as np
import pytest

import resample_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(pkg):
    return rc.make_case(pkg)


@pytest.mark.parametrize("extrapolate", (0, 1))
def test_device_pointers_on_a_stream_equal_host_pointers(hip_model, pkg, case, extrapolate):
    import torch
    k, cap = case, pkg._capi
    code, host, st_h = rc.call(pkg, hip_model, k, extrapolate)
    assert code == 0, hip_model._lib.plh_last_error()
    stream = torch.cuda.Stream()
    code, dev, st_d = rc.call(pkg, hip_model, k, extrapolate, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0, hip_model._lib.plh_last_error()
    assert np.array_equal(host, dev, equal_nan=True) and (st_h == 0).all() and (st_d == 0).all()
    ref = rc.fitpack_reference(k, extrapolate)
    nanq = np.isnan(k.tq)
    assert np.isnan(dev[:, nanq]).all() and np.isfinite(dev[:, ~nanq]).all()
    for c in range(k.n):
        err = rc.scaled_error(k, dev, ref, c, rc.mild(k, c) if extrapolate else None)
        print("extrapolate %d cell %d: %.3e of max|column| (tolerance %.1e)" % (extrapolate, c, err, rc.TOL))
        assert err <= rc.TOL, (c, err)
    for w in (1, 65):                                                                                  # a width of one lane, a width of a tile and one column
        code, part, _ = rc.call(pkg, hip_model, k, extrapolate, width=w, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
        assert code == 0 and np.array_equal(part, dev[:, :, :w], equal_nan=True), w


def test_ensemble_in_hbm_against_the_single_cell_spline(hip_model, pkg):
    import torch
    p, n = hip_model, 8
    rng = np.random.default_rng(2)
    scale = 2.0 ** (2 * rng.random((n, 2)) - 1)
    Th = pkg.theta_matrix(p, n, {"D_sp": p.θ["D_sp"] * scale[:, 0], "k_p": p.θ["k_p"] * scale[:, 1]})
    proto = [{"I": 2.0, "tf": 1000.0, "SOC_max": 0.2}, {"I": -1.0, "tf": 100.0}]
    stream = torch.cuda.Stream()
    ens = pkg.simulate_ensemble(p, torch.from_numpy(Th).cuda(), proto, SOC=0.1, device=True, outputs="all", stream=stream.cuda_stream)
    torch.cuda.synchronize()
    n_pts = ens.n_pts.cpu().numpy()
    t = ens.t.cpu().numpy()
    last = np.array([t[i, n_pts[i] - 1] for i in range(n)])
    first = int(np.argmin(last))                                                                       # the cell that ends first: a query behind its end is inside every other cell
    # outside the points, but mildly (half an end step: tests/resample_cases.py on far extrapolation): before every cell's second point, behind the first end
    outside = [-0.5 * t[:, 1].min(), last[first] + 0.5 * (last[first] - t[first, n_pts[first] - 2])]
    tq = np.concatenate([rng.uniform(0.0, last[first], 20), outside, [t[first, 5], ens.run_info[first, 0]["t_end"]]])
    tq = tq[rng.permutation(len(tq))]
    for bc in ("interpolate", "extrapolate"):
        res = ens(tq, interp_bc=bc)
        assert isinstance(res.Y_all, torch.Tensor) and res.Y_all.is_cuda and res.Y_all.shape == (n, len(res.t), p.N.tot) and res.V.shape == (n, len(res.t))
        torch.cuda.synchronize()
        assert (res.status.cpu().numpy() == 0).all()
        assert torch.equal(res.section("c_e"), res.Y_all[:, :, p.ind["c_e"]])
        for i in (first, (first + 3) % n):
            one = ens[i](res.t, interp_bc=bc)
            m = int(ens.n_pts[i])
            for nm in ("V", "I", "SOC", "Y_all"):
                got, ref = getattr(res, nm)[i].cpu().numpy().reshape(len(res.t), -1), getattr(one, nm).reshape(len(res.t), -1)
                sc = np.abs(getattr(ens, nm)[i, :m].cpu().numpy().reshape(m, -1)).max(axis=0)
                keep = sc > 0
                assert np.array_equal(got[:, ~keep], ref[:, ~keep])
                worst = float((np.abs(got - ref)[:, keep] / sc[keep]).max())
                print("%s cell %d %s: %.3e of max|column| (tolerance %.1e)" % (nm, i, bc, worst, rc.TOL))
                assert worst <= rc.TOL, (nm, i, bc, worst)


def test_chunked_workspace_gives_the_same_bits(hip_model, pkg, monkeypatch):
    import torch
    cap = pkg._capi
    pts = ((5, 9), (1, 2), (40, 3), (4, 4), (2, 30), (7, 100), (3, 3), (64, 64), (2, 2))
    k = rc.make_case(pkg, cell_points=pts, width=70, seed=5)
    stream = torch.cuda.Stream()
    code, whole, st = rc.call(pkg, hip_model, k, 1, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and (st == 0).all()
    monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(2 * 8 * k.max_pts * 70 + 8192))                    # two cells' slopes: five chunks
    code, got, st = rc.call(pkg, hip_model, k, 1, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and (st == 0).all() and np.array_equal(got, whole, equal_nan=True)
    code, got, st = rc.call(pkg, hip_model, k, 1)                                                      # and through host pointers
    assert code == 0 and np.array_equal(got, whole, equal_nan=True)
