"""fit_ensemble: the whole fit -- sensitivity integration, ens.lsq, plh_lm_step -- on the wave-emulator build (no GPU) and in HBM on the GPU.  Every recorded iteration is
replayed through the restatement of tests/lm_cases.py with the inputs the kernel saw, within its bounds; the GPU fit must end no worse than the truth."""
import numpy as np
import pytest

import lm_cases as lm
import parity

KEYS = ["D_sp", "k_p"]


def test_fit_ensemble_on_the_emulator(emu_model, pkg):
    p, n = emu_model, 2
    cols = [p.θ_keys.index(k) for k in KEYS]
    proto = [{"I": -1.0, "tf": 60.0}]
    t = np.linspace(2.0, 58.0, 12)
    truth = pkg.theta_matrix(p, 1)
    V_data = np.asarray(pkg.simulate_ensemble(p, truth, proto, SOC=0.9)(t, fields="V").V[0])
    Theta0 = pkg.theta_matrix(p, n)
    Theta0[:, cols] *= np.array([[1.3, 0.8], [0.8, 1.25]])
    keep = Theta0.copy()
    tf = {k: "log" for k in KEYS}
    res = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, SOC=0.9, transform=tf, max_iter=6, history=True)
    assert lm.same_bits(Theta0, keep)                                                       # the input is not modified
    other = np.setdiff1d(np.arange(Theta0.shape[1]), cols)
    assert lm.same_bits(np.ascontiguousarray(res.theta[:, other]), np.ascontiguousarray(keep[:, other]))
    assert res.keys == KEYS and 2 <= res.n_iter <= 7 and len(res.history) == res.n_iter
    worst = lm.replay(res.history, cols, [lm.LOG, lm.LOG], None, None, what="emulator fit")
    first = res.history[0]["cost"]
    print("emulator fit: %d integrations, states %s, cost %s -> %s, replay at %s of the bounds" % (res.n_iter, res.state.tolist(), first.tolist(), res.cost.tolist(), worst))
    assert (res.cost <= 1e-2 * first).all()
    assert lm.same_bits(np.ascontiguousarray(res.theta[:, cols]), res.history[-1]["after"]["theta_cur"])
    # refusals
    with pytest.raises(ValueError):
        pkg.fit_ensemble(p, Theta0, proto, list(p.θ_keys[:9]), t, V_data)
    with pytest.raises(ValueError):
        pkg.fit_ensemble(p, Theta0, proto, ["D_sp", "no_such_key"], t, V_data)
    with pytest.raises(ValueError):
        pkg.fit_ensemble(p, Theta0, proto, KEYS, t)
    with pytest.raises(ValueError):
        pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, transform={"D_sp": "sqrt"})
    with pytest.raises(ValueError):
        pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data[:5])                             # what ens.lsq refuses


@pytest.mark.gpu
def test_device_pointers_on_a_stream_equal_host_pointers(hip_model, pkg):
    """accepting, rejecting and failed trials, a LOG / LINEAR mix and bounds that hold and clamp, 70 cells, k = 8: PLH_DEVICE on a stream of the caller's against PLH_HOST"""
    import torch
    cap, n, k = pkg._capi, 70, 8
    theta, cols = lm.make_theta(n, k, 201)
    tf = np.array([lm.LOG, lm.LINEAR] * 4, np.int32)
    lo, hi = np.full((n, k), 0.05), np.full((n, k), 20.0)
    lo[::3, 1] = theta[::3, cols[1]]                                                        # at a bound: held or free, as the gradient says
    hi[1::3, 3] = theta[1::3, cols[3]] * (1 + 1e-4)                                         # a step of any size up overshoots
    fits = [lm.make_fit(n, k, 202, cost_scale=1e-6)]
    status = [np.zeros(n, np.int32)]
    stream = torch.cuda.Stream()
    st_h, st_d, th_h = lm.State(n, k), None, theta.copy()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(theta=dev(theta), lo=dev(lo), hi=dev(hi), nrun=torch.zeros(1, dtype=torch.int32, device="cuda"), **{a: dev(getattr(st_h, a)) for a in lm.STATE_ARRAYS})
    ci, ti = np.ascontiguousarray(cols, dtype=np.int32), tf
    for it, phase in enumerate((lm.FIRST, lm.STEP, lm.STEP)):
        if it:                                                                              # the trials of the host run are judged: accept / reject / failed / NaN in grad
            kinds = [("accept", "reject", "failed", "nan_grad")[(c + it) % 4] for c in range(n)]
            c2, g2, H2 = lm.make_fit(n, k, 202 + it, cost_scale=1e-6)
            run = st_h.state == lm.RUNNING
            tgt = np.where(np.array([x in ("accept", "nan_grad") for x in kinds]), st_h.cost_cur - 0.5 * st_h.pred, st_h.cost_cur + st_h.pred)
            tgt = np.where(run, tgt, 1.0)
            c2, g2, H2 = lm.with_cost(c2, g2, H2, tgt)
            s2 = np.zeros(n, np.int32)
            for c, x in enumerate(kinds):
                if x == "failed":
                    s2[c], c2[c] = 1, np.nan
                if x == "nan_grad":
                    g2[c, k - 1] = np.nan
            fits.append((c2, g2, H2)); status.append(s2)
        cost, grad, JtJ = fits[it]
        ref, _ = lm.run(hip_model, th_h, cols, tf, lo, hi, cost, grad, JtJ, status[it], st_h, phase, None, "host pointers, call %d" % it)
        f = [dev(a) for a in (cost, grad, JtJ, status[it])]
        rc = hip_model._lib.plh_lm_step(hip_model._h, n, theta.shape[1], d["theta"].data_ptr(), k, ci.ctypes.data, ti.ctypes.data, d["lo"].data_ptr(), d["hi"].data_ptr(), 1,
                                        f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), *[d[a].data_ptr() for a in lm.STATE_ARRAYS[:6]],
                                        *[d[a].data_ptr() for a in lm.STATE_ARRAYS[6:]], None, phase, d["nrun"].data_ptr(), cap.PLH_DEVICE, stream.cuda_stream)
        assert rc == 0, hip_model._lib.plh_last_error()
        stream.synchronize()
        assert lm.same_bits(d["theta"].cpu().numpy(), th_h), "theta, call %d" % it
        for a in lm.STATE_ARRAYS:
            assert lm.same_bits(d[a].cpu().numpy(), getattr(st_h, a)), (a, it)
        assert int(d["nrun"].cpu()[0]) == ref[2]
        if it == 0:
            held = np.array([i["held"][1] for i in ref[3]])
            clamped = np.array([i["clamped"][3] for i in ref[3]])
            assert held[::3].any() and clamped[1::3].any()


@pytest.mark.gpu
def test_fit_recovers_parameters_in_hbm(hip_model, pkg, O):
    import torch
    p, n = hip_model, 16
    cols = [p.θ_keys.index(k) for k in KEYS]
    proto = [{"I": 1.0, "V_max": 3.95, "tf": 600.0}, {"V": "hold", "I_min": 0.3, "tf": 300.0}]     # the CC-CV protocol of INTEGRATION.md, shortened: from SOC 0.5, V_max after ~460 s
    o = pkg.Opts(); o.reltol, o.abstol, o.maxiters = parity.TIGHT["reltol"], parity.TIGHT["abstol"], 200000
    truth = pkg.theta_matrix(p, 1)
    ro = O.simulate(p.variant, truth[0], 0.5, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(maxiters=1000000, **parity.TIGHT), max_out=200000)
    assert ro["rc"] == 0 and ro["runs"][0]["flag"] == 2, ro["runs"]                          # the CC leg ends on V_max
    t_cc, t_end = ro["runs"][0]["t_end"], ro["runs"][1]["t_end"]
    t = np.concatenate([np.linspace(0.05 * t_cc, 0.95 * t_cc, 12), np.linspace(t_cc + 0.1 * (t_end - t_cc), t_cc + 0.9 * (t_end - t_cc), 8)])
    in_cc = t < t_cc
    keep = np.concatenate([[True], np.diff(ro["t"]) > 0])                                    # (the join appears twice)
    V_data, I_data = np.interp(t, ro["t"][keep], ro["V"][keep]), np.interp(t, ro["t"][keep], ro["I"][keep])
    # measurement noise of the size the weights state (1 mV, 0.01 C), from a fixed seed.  Without it the cost at the truth is what the library and the oracle differ by
    # (3.4e-6 here), which moves by a few per cent with the step sequences of the adaptive integration: "no worse than the truth" would then compare two noises (measured:
    # thirteen of sixteen cells ended at 3.42e-6 .. 3.44e-6 against 3.39e-6 at the truth, parameters within 6.6e-5 of it).  With it the cost at the truth is about n_q / 2 = 10
    # and the minimiser lies about k / 2 = 1 below it: five orders above that noise.
    sV, sI = 1e-3, 1e-2
    rng = np.random.default_rng(5)
    V_data, I_data = V_data + sV * rng.standard_normal(len(t)), I_data + sI * rng.standard_normal(len(t))
    wV, wI = in_cc / sV, (~in_cc) / sI
    Theta0 = pkg.theta_matrix(p, n)
    Theta0[:, cols] *= 2.0 ** rng.uniform(-0.5, 0.5, size=(n, 2))
    stream = torch.cuda.Stream()
    Th_d = torch.from_numpy(Theta0).cuda()
    tf = {k: "log" for k in KEYS}
    lmo = dict(ftol=1e-10)
    res = pkg.fit_ensemble(p, Th_d, proto, KEYS, t, V_data, wV, I_data, wI, SOC=0.5, opts=o, transform=tf, max_iter=15, device=True, stream=stream.cuda_stream, lm=lmo, history=True)
    stream.synchronize()
    for a in (res.theta, res.cost, res.grad, res.JtJ, res.state, res.lam, res.n_accept, res.n_reject):
        assert isinstance(a, torch.Tensor) and a.is_cuda
    assert lm.same_bits(Th_d.cpu().numpy(), Theta0)
    worst = lm.replay(res.history, cols, [lm.LOG, lm.LOG], None, None, lmo, what="fit in HBM")
    state, cost = res.state.cpu().numpy(), res.cost.cpu().numpy()
    assert np.isin(state, (lm.CONV_F, lm.CONV_X, lm.CONV_G, lm.MAXIT)).all(), state
    at_truth = pkg.simulate_ensemble(p, torch.from_numpy(truth).cuda(), proto, SOC=0.5, opts=o, device=True, sens=KEYS, sens_outputs=("V", "I")).lsq(t, V_data, wV, I_data=I_data, I_weights=wI)
    torch.cuda.synchronize()
    c_true = float(at_truth.cost.cpu()[0])
    rel = np.abs(res.theta.cpu().numpy()[:, cols] / truth[0, cols] - 1)
    print("fit in HBM: %d integrations, states %s, final cost %s, cost at the truth %.6g, |theta / truth - 1| <= %.3g, replay at %s of the bounds"
          % (res.n_iter, state.tolist(), cost.tolist(), c_true, rel.max(), worst))
    assert (cost <= c_true * (1 + 10 * lmo["ftol"])).all()
