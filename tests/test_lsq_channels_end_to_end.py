"""EnsembleSolution.lsq over the voltage and the current channel of a CC / V-hold ensemble integrated with sens_outputs=("V", "I"): the Python layer on a host ensemble
(wave emulator), and eight cells in HBM on the GPU.  The yardstick of the sums is the sum of two single-channel plh_lsq calls on the same arrays, within the summed bounds of
lsq_cases (each call is held to its own bounds by tests/test_lsq.py / test_gpu_lsq.py); the zero-residual bound is lsq_cases.bounds at r = 0."""
import numpy as np
import pytest

import lsq_cases as lc
import resample_cases as rc

PROTO = [{"I": 2.0, "tf": 300, "V_max": 5.0}, {"V": "hold", "tf": 200, "V_max": 5.0, "I_min": 0.0}]          # (case A of tests/test_sens_channels.py)
KEYS = ["D_sp", "k_n"]


def host_case(ens, tq, chan):
    """the ensemble's arrays (host copies) as a resample case of width 1 + K: the channel's curve, then the rows of its sensitivities"""
    H = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    t, n_pts = H(ens.t), H(ens.n_pts)
    n, nr = t.shape[0], len(ens.run_names)
    k = rc.Case()
    k.n, k.n_runs, k.max_pts, k.width, k.tq = n, nr, t.shape[1], 1 + len(KEYS), tq
    k.t, k.n_pts, k.run_info = t, n_pts, ens.run_info
    k.src = np.concatenate([H(getattr(ens, chan))[:, :, None], H(getattr(ens, {"V": "dV_dtheta", "I": "dI_dtheta"}[chan])).transpose(0, 2, 1)], axis=2)
    k.runs = [[(int(sum(ens.run_info[c, :r]["iterations"])), int(ens.run_info[c, r]["iterations"])) for r in range(nr)] for c in range(n)]
    return k


def summed_bounds(ens, tq, data, weights):
    """per cell: the sum over the channels of lsq_cases.bounds, from the scipy-resampled arrays of the ensemble itself"""
    out = []
    ks = {ch: host_case(ens, tq, ch) for ch in data}
    S = {ch: rc.fitpack_reference(ks[ch], 0) for ch in data}
    for c in range(ks["V"].n):
        b = dict(cost=0.0, grad=0.0, JtJ=0.0)
        for ch in data:
            ref = lc.reference(S[ch][c], data[ch], weights[ch])
            bc = lc.bounds(ks[ch], c, len(KEYS), ref, weights[ch])
            for nm in b:
                b[nm] = b[nm] + bc[nm]
        out.append(b)
    return out


def check_python_layer(pkg, p, device):
    n = 8 if device else 2
    rng = np.random.default_rng(3)
    scale = 2.0 ** (0.5 * (2 * rng.random((n, 2)) - 1))
    scale[0] = 1.0
    Th = pkg.theta_matrix(p, n, {"D_sp": p.θ["D_sp"] * scale[:, 0], "k_n": p.θ["k_n"] * scale[:, 1]})
    H = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if device:
        import torch
        Th = torch.from_numpy(Th).cuda()
    ens = pkg.simulate_ensemble(p, Th, PROTO, SOC=0.2, sens=KEYS, sens_outputs=("V", "I"), device=device)
    assert ens.dT_avg_dtheta is None and tuple(ens.dI_dtheta.shape) == tuple(ens.dV_dtheta.shape)
    assert (ens.run_info["flag"] >= 0).all()
    tq = np.linspace(5.0, 495.0, 40)                                   # both legs
    res = ens(tq, fields=("V", "I"))
    V0, I0 = res.V[0], res.I[0]                                        # cell 0's own curves (device: stay in HBM)
    wV, wI = 0.5 + rng.random(len(tq)), 2.0 * (0.5 + rng.random(len(tq)))
    both = ens.lsq(tq, V0, weights=wV, I_data=I0, I_weights=wI, resid=True)
    onlyV = ens.lsq(tq, V0, weights=wV, resid=True)
    onlyI = ens.lsq(tq, I_data=I0, I_weights=wI, resid=True)
    assert both.channels == ["V", "I"] and onlyV.channels == ["V"] and onlyI.channels == ["I"] and both.keys == KEYS
    assert both.resid_T_avg is None and onlyV.resid_I is None and onlyI.resid is None
    assert (H(both.status) == 0).all()
    data, weights = {"V": H(V0), "I": H(I0)}, {"V": wV, "I": wI}
    bnd = summed_bounds(ens, tq, data, weights)
    # cell 0 against its own curves: zero residuals to rounding
    print("cell 0 against its own curves: cost %.3e (bound %.3e)" % (H(both.cost)[0], bnd[0]["cost"]))
    assert H(both.cost)[0] <= bnd[0]["cost"]
    # the other cells: the fused call against the sum of the two single-channel calls, within the summed bounds
    assert np.array_equal(H(both.resid), H(onlyV.resid)) and np.array_equal(H(both.resid_I), H(onlyI.resid_I))
    for c in range(1, n):
        for nm in ("cost", "grad", "JtJ"):
            d = np.abs(H(getattr(both, nm))[c] - (H(getattr(onlyV, nm))[c] + H(getattr(onlyI, nm))[c]))
            print("cell %d %s: |fused - (V + I)| / summed bound %.3g" % (c, nm, float(np.max(d / bnd[c][nm]))))
            assert (d <= bnd[c][nm]).all(), (c, nm, d, bnd[c][nm])
        assert H(both.cost)[c] > 1e3 * H(both.cost)[0]
    # Over the hold leg alone the voltage is the input: for the cell the data come from, the voltage channel has nothing to say there (its residual is the rounding of the
    # resampling, whatever the current does), while a current that differs from the measured one by 0.01 C pulls on the parameters through dI/dtheta.  (dV/dtheta of a
    # V = :hold leg is a constant, not 0 -- the held value is the end voltage of the CC run -- so for the OTHER cells, whose held voltage differs from the data, the voltage
    # channel does carry a gradient there: this statement is about cell 0.)
    th = np.linspace(310.0, 490.0, 19)
    rh = ens(th, fields=("V", "I"))
    gV = H(ens.lsq(th, H(rh.V[0])).grad)[0]
    gI = H(ens.lsq(th, I_data=H(rh.I[0]) + 0.01).grad)[0]
    print("hold leg, cell 0: |grad| of the V-only call %s, of the I-only call %s" % (np.abs(gV).tolist(), np.abs(gI).tolist()))
    assert (np.abs(gI) > 0).all() and (np.abs(gV) <= 1e-8 * np.abs(gI)).all()
    return ens


def test_ensemble_lsq_channels_on_the_host(emu_model, pkg):
    ens = check_python_layer(pkg, emu_model, device=False)
    tq = np.linspace(5.0, 495.0, 12)
    d = np.zeros(len(tq))
    with pytest.raises(ValueError, match="at least one channel"):
        ens.lsq(tq)
    with pytest.raises(ValueError, match="no per-point T_avg"):
        ens.lsq(tq, T_avg_data=d)
    with pytest.raises(ValueError, match="I_weights"):
        ens.lsq(tq, d, I_data=d, I_weights=d[:-1])
    onlyV = pkg.simulate_ensemble(emu_model, np.asarray(emu_model.theta_vector())[None, :].copy(), [{"I": -1.0, "tf": 20.0}], SOC=0.9, sens=["D_sp"])
    assert onlyV.dI_dtheta is None
    with pytest.raises(ValueError, match="sens_outputs"):
        onlyV.lsq(np.array([5.0, 10.0]), I_data=np.zeros(2))
    plain = pkg.simulate_ensemble(emu_model, np.asarray(emu_model.theta_vector())[None, :].copy(), [{"I": -1.0, "tf": 20.0}], SOC=0.9)
    mis = plain.lsq(np.array([5.0, 10.0]), I_data=np.full(2, -1.0))                                        # the misfit-only call on the current channel
    assert mis.grad is None and mis.channels == ["I"] and mis.cost[0] < 1e-20


@pytest.mark.gpu
def test_ensemble_lsq_channels_in_hbm(hip_model, pkg):
    import torch
    ens = check_python_layer(pkg, hip_model, device=True)
    assert isinstance(ens.dI_dtheta, torch.Tensor) and ens.dI_dtheta.is_cuda
