"""fit_ensemble(groups=...): consecutive cells share the fitted keys, one experiment per member -- sensitivity integration, ens.lsq, plh_lsq_group, plh_lm_step on the groups,
plh_group_scatter -- on the wave-emulator build (no GPU) and in HBM on the GPU.  Every recorded iteration is replayed through the restatement of tests/lm_cases.py with the
group-level inputs the kernel saw, every recorded group fit is the restatement of tests/lsq_group_cases.py on the recorded member fits, bit for bit; the GPU fit must end no
worse than the truth."""
import numpy as np
import pytest

import lm_cases as lm
import lsq_group_cases as gc
import parity

KEYS = ["D_sp", "k_p"]
RESULT_ARRAYS = ("theta", "cost", "grad", "JtJ", "state", "lam", "n_accept", "n_reject")


def check_group_history(res, off, cols, members):
    for it, rec in enumerate(res.history):
        m = rec["member"]
        ref = gc.sum_reference(off, m["cost"], m["grad"], m["JtJ"], m["status"])
        for a, b in zip((rec["cost"], rec["grad"], rec["JtJ"]), ref):
            assert gc.same_bits_nan(a, b), it
        assert np.array_equal(rec["status"], ref[3]), it
        # after the scatter every member holds its group's row in the keys
        assert np.ascontiguousarray(rec["Theta"][:, cols]).tobytes() == np.ascontiguousarray(np.repeat(rec["theta_after"][:, cols], members, axis=0)).tobytes(), it


def test_grouped_fit_on_the_emulator(emu_model, pkg):
    p, n, ng = emu_model, 4, 2
    cols = [p.θ_keys.index(k) for k in KEYS]
    groups = np.array([0, 0, 1, 1])
    proto = [{"I": np.array([-0.5, -1.0, -0.5, -1.0]), "tf": 60.0}]     # one experiment per member
    t = np.linspace(2.0, 58.0, 12)
    V_data = np.ascontiguousarray(pkg.simulate_ensemble(p, pkg.theta_matrix(p, n), proto, SOC=0.9)(t, fields="V").V)
    assert V_data.shape == (4, 12)
    Theta0 = pkg.theta_matrix(p, n)
    Theta0[:, cols] *= np.array([[1.3, 0.8], [0.7, 1.1], [0.8, 1.25], [1.2, 0.9]])      # the members disagree at the start: the first member's values count
    keep = Theta0.copy()
    tf = {k: "log" for k in KEYS}
    res = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, SOC=0.9, transform=tf, max_iter=6, history=True, groups=groups)
    assert lm.same_bits(Theta0, keep)                                                       # the input is not modified
    assert np.array_equal(res.group_off, [0, 2, 4]) and res.keys == KEYS and 2 <= res.n_iter <= 7 and len(res.history) == res.n_iter
    assert res.theta.shape == Theta0.shape and res.cost.shape == (ng,) and res.grad.shape == (ng, 2) and res.JtJ.shape == (ng, 2, 2)
    for a in (res.state, res.lam, res.n_accept, res.n_reject):
        assert a.shape == (ng,)
    first = res.history[0]
    assert first["theta_before"].shape == (ng, Theta0.shape[1])
    assert lm.same_bits(np.ascontiguousarray(first["theta_before"][:, cols]), np.ascontiguousarray(keep[[0, 2]][:, cols]))      # a group starts at its first member's keys
    worst = lm.replay(res.history, cols, [lm.LOG, lm.LOG], None, None, what="grouped emulator fit")
    check_group_history(res, res.group_off, cols, 2)
    print("grouped emulator fit: %d integrations, states %s, cost %s -> %s, replay at %s of the bounds" % (res.n_iter, res.state.tolist(), first["cost"].tolist(), res.cost.tolist(), worst))
    assert (res.cost <= 1e-2 * first["cost"]).all()
    # the members of a group have identical bits in the keys: the group's theta_cur; every other column is Theta0's
    assert np.ascontiguousarray(res.theta[:, cols]).tobytes() == np.repeat(res.history[-1]["after"]["theta_cur"], 2, axis=0).tobytes()
    other = np.setdiff1d(np.arange(Theta0.shape[1]), cols)
    assert lm.same_bits(np.ascontiguousarray(res.theta[:, other]), np.ascontiguousarray(keep[:, other]))
    # by_group on the result of ens.lsq is plh_lsq_group
    ens = pkg.simulate_ensemble(p, Theta0, proto, SOC=0.9, sens=KEYS)
    fit = ens.lsq(t, V_data)
    gf = fit.by_group(groups)
    ref = gc.sum_reference(res.group_off, fit.cost, fit.grad, fit.JtJ, fit.status)
    assert gc.same_bits_nan(gf.cost, ref[0]) and gc.same_bits_nan(gf.grad, ref[1]) and gc.same_bits_nan(gf.JtJ, ref[2]) and np.array_equal(gf.status, ref[3])
    assert gf.resid is None and gf.resid_I is None and gf.resid_T_avg is None and gf.keys == KEYS


def test_groups_of_one_are_the_fit_without_groups(emu_model, pkg):
    p, n = emu_model, 2
    cols = [p.θ_keys.index(k) for k in KEYS]
    proto = [{"I": -1.0, "tf": 60.0}]
    t = np.linspace(2.0, 58.0, 12)
    V_data = np.asarray(pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), proto, SOC=0.9)(t, fields="V").V[0])
    Theta0 = pkg.theta_matrix(p, n)
    Theta0[:, cols] *= np.array([[1.3, 0.8], [0.8, 1.25]])
    kw = dict(SOC=0.9, transform={k: "log" for k in KEYS}, max_iter=4)
    a = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, **kw)
    b = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, groups=np.arange(n), **kw)
    assert a.n_iter == b.n_iter and a.group_off is None and np.array_equal(b.group_off, [0, 1, 2])
    for x in RESULT_ARRAYS:
        assert lm.same_bits(np.ascontiguousarray(getattr(a, x)), np.ascontiguousarray(getattr(b, x))), x


def test_bad_groups_are_refused(emu_model, pkg):
    p, n = emu_model, 4
    proto = [{"I": -1.0, "tf": 60.0}]
    t = np.linspace(2.0, 58.0, 12)
    Theta0 = pkg.theta_matrix(p, n)
    V_data = np.full(12, 4.0)
    for what, g in (("decreasing", [0, 1, 0, 1]), ("a gap", [0, 0, 2, 2]), ("not from 0", [1, 1, 2, 2]), ("wrong length", [0, 0, 1]), ("too long", [0, 0, 1, 1, 1]),
                    ("not 1-D", [[0, 0, 1, 1]]), ("not integers", [0.0, 0.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, groups=np.array(g))
        with pytest.raises(ValueError):
            pkg.group_offsets(np.array(g), n)
    assert np.array_equal(pkg.group_offsets(np.array([0, 0, 0, 1]), 4), [0, 3, 4])
    with pytest.raises(ValueError):                                                         # bounds of a grouped fit are per group
        pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, groups=np.array([0, 0, 1, 1]), bounds={"k_p": (np.zeros(n), None)})


@pytest.mark.gpu
def test_device_pointers_on_a_stream_equal_host_pointers(hip_model, pkg):
    """plh_lsq_group and plh_group_scatter, the 326-cell shape with k = 8: PLH_DEVICE on a stream of the caller's against PLH_HOST and against the restatement"""
    import torch
    cap, k, nth = pkg._capi, 8, 11
    n, ng = int(np.sum(gc.SIZES)), len(gc.SIZES)
    off = gc.offsets(gc.SIZES)
    cost, grad, JtJ = gc.make_fits(n, k, 18)
    status = np.zeros(n, np.int32)
    cost[70], status[200], grad[131, 7] = np.nan, 1, np.inf
    ref = gc.sum_reference(off, cost, grad, JtJ, status)
    out = gc.sum_outputs(ng, k)
    assert gc.call_sum(hip_model, off, cost, grad, JtJ, status, out) == 0, hip_model._lib.plh_last_error()
    for a, b in zip((out["g_cost"], out["g_grad"], out["g_JtJ"]), ref):
        assert gc.same_bits_nan(a, b)
    assert np.array_equal(out["g_status"], ref[3])
    stream = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_in = [dev(a) for a in (cost, grad, JtJ, status)]
    d_out = [torch.empty(ng, dtype=torch.float64, device="cuda"), torch.empty(ng, k, dtype=torch.float64, device="cuda"), torch.empty(ng, k, k, dtype=torch.float64, device="cuda"),
             torch.empty(ng, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    lib, h = hip_model._lib, hip_model._h
    for _ in range(2):                                                                      # (the second call finds the offsets on the device)
        rc = lib.plh_lsq_group(h, n, ng, off.ctypes.data, k, *[a.data_ptr() for a in d_in], *[a.data_ptr() for a in d_out], cap.PLH_DEVICE, stream.cuda_stream)
        assert rc == 0, lib.plh_last_error()
    stream.synchronize()
    for a, b in zip(d_out[:3], (out["g_cost"], out["g_grad"], out["g_JtJ"])):
        assert gc.same_bits_nan(a.cpu().numpy(), b)
    assert np.array_equal(d_out[3].cpu().numpy(), out["g_status"])
    # the scatter
    cols = np.array([9, 2, 10, 0, 5, 7, 1, 4], np.int32)
    theta = np.ascontiguousarray(1000.0 + np.arange(n * nth, dtype=np.float64).reshape(n, nth))
    g_theta = np.ascontiguousarray(-1.0 - np.arange(ng * nth, dtype=np.float64).reshape(ng, nth))
    want = gc.scatter_reference(off, cols, g_theta, theta)
    d_theta, d_g = dev(theta), dev(g_theta)
    torch.cuda.synchronize()
    assert gc.call_scatter(hip_model, off, cols, g_theta, theta) == 0, lib.plh_last_error()
    assert theta.tobytes() == want.tobytes()
    rc = lib.plh_group_scatter(h, n, ng, off.ctypes.data, nth, k, cols.ctypes.data, d_g.data_ptr(), d_theta.data_ptr(), cap.PLH_DEVICE, stream.cuda_stream)
    assert rc == 0, lib.plh_last_error()
    stream.synchronize()
    assert d_theta.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.gpu
def test_grouped_fit_recovers_parameters_in_hbm(hip_model, pkg):
    import torch
    p, ng, m = hip_model, 8, 3
    n = ng * m
    cols = [p.θ_keys.index(k) for k in KEYS]
    groups = np.repeat(np.arange(ng), m)
    proto = [{"I": np.tile([-0.5, -1.0, -2.0], ng), "tf": 300.0}]      # three C-rates per group
    o = pkg.Opts(); o.reltol, o.abstol, o.maxiters = parity.TIGHT["reltol"], parity.TIGHT["abstol"], 200000
    t = np.linspace(15.0, 285.0, 16)
    truth = pkg.theta_matrix(p, n)
    # data: the library's own truth run of every member plus measurement noise of the size the weights state (1 mV), from a fixed seed.  As in
    # test_lm_fit.py::test_fit_recovers_parameters_in_hbm: the cost of a member at the truth is about n_q / 2 = 8, of a group about 24, and the minimiser lies about k / 2 = 1
    # below it -- orders of magnitude above what the step sequences of the adaptive integration move the cost by
    sV = 1e-3
    rng = np.random.default_rng(6)
    V_true = pkg.simulate_ensemble(p, truth, proto, SOC=0.9, opts=o)(t, fields="V").V
    V_data = np.ascontiguousarray(np.asarray(V_true) + sV * rng.standard_normal((n, len(t))))
    wV = np.full(len(t), 1.0 / sV)
    Theta0 = truth.copy()
    Theta0[:, cols] *= np.repeat(2.0 ** rng.uniform(-0.5, 0.5, size=(ng, 2)), m, axis=0)
    stream = torch.cuda.Stream()
    Th_d = torch.from_numpy(Theta0).cuda()
    tf = {k: "log" for k in KEYS}
    lmo = dict(ftol=1e-10)
    res = pkg.fit_ensemble(p, Th_d, proto, KEYS, t, V_data, wV, SOC=0.9, opts=o, transform=tf, max_iter=20, device=True, stream=stream.cuda_stream, lm=lmo, history=True, groups=groups)
    stream.synchronize()
    for a in (res.cost, res.grad, res.JtJ, res.state, res.lam, res.n_accept, res.n_reject):
        assert isinstance(a, torch.Tensor) and a.is_cuda and a.shape[0] == ng
    assert isinstance(res.theta, torch.Tensor) and res.theta.is_cuda and tuple(res.theta.shape) == Theta0.shape
    assert lm.same_bits(Th_d.cpu().numpy(), Theta0)
    worst = lm.replay(res.history, cols, [lm.LOG, lm.LOG], None, None, lmo, what="grouped fit in HBM")
    check_group_history(res, res.group_off, cols, m)
    state, cost = res.state.cpu().numpy(), res.cost.cpu().numpy()
    th = res.theta.cpu().numpy()
    assert np.ascontiguousarray(th[:, cols]).tobytes() == np.repeat(res.history[-1]["after"]["theta_cur"], m, axis=0).tobytes()
    assert np.isin(state, (lm.CONV_F, lm.CONV_X, lm.CONV_G, lm.MAXIT)).all(), state
    at_truth = pkg.simulate_ensemble(p, torch.from_numpy(truth).cuda(), proto, SOC=0.9, opts=o, device=True, sens=KEYS).lsq(t, V_data, wV).by_group(groups)
    torch.cuda.synchronize()
    c_true = at_truth.cost.cpu().numpy()
    assert c_true.shape == (ng,)
    rel = np.abs(th[:, cols] / truth[:, cols] - 1)
    print("grouped fit in HBM: %d integrations, states %s, final cost %s, cost at the truth %s, |theta / truth - 1| <= %.3g, replay at %s of the bounds"
          % (res.n_iter, state.tolist(), cost.tolist(), c_true.tolist(), rel.max(), worst))
    assert (cost <= c_true * (1 + 10 * lmo["ftol"])).all()
