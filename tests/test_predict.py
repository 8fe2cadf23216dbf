"""plh_predict / EnsembleSolution.predict on the wave emulator (the product's device and host source on the CPU): the resampled curves, their resampled sensitivities and
the delta-method variance against the scipy-built yardstick within the bounds tests/predict_cases.py derives; channels, NULL outputs, held and unseen keys, failed cells,
NaN queries, saved times, grouped covariances, the argument checks, and the Python front end."""
import copy

import numpy as np
import pytest

import predict_cases as pc
import resample_cases as rc


@pytest.fixture(scope="module")
def problems(pkg):
    return {name: pc.make_problem(pkg, name) for name in pc.CASES}


def test_restatement_sits_far_inside_the_bounds(problems):
    """where the numpy float64 restatement (resample_cases.restatement, then the two sums in the stated order) sits in the bounds, every K, cell and extrapolate value: no
    code under test involved.  pred / dpred: <= 0.01, TOL's definition.  var: <= 0.1 ((2 K + 2) / (64 K) <= 0.0625 for the sums, 0.01 for the propagated part)."""
    worst = {}
    for name, pb in problems.items():
        for ex in (0, 1):
            mine = rc.restatement(pb.k, ex)
            for K in pc.KS:
                for c in range(pb.k.n):
                    M = pb.cov[K][c]
                    ref = pc.reference(pb.S[ex][c], K, M)
                    got = dict(pred=mine[c][:, 0], dpred=np.ascontiguousarray(mine[c][:, 1:1 + K].T))
                    got["var"] = pc.restated_var(M, got["dpred"])
                    rat = pc.ratios(got, ref, pc.bounds(pb.k, c, K, ref, M), pc.compared(pb.k, c, ex))
                    print("%s K %d extrapolate %d cell %d: restatement at " % (name, K, ex, c) + " ".join("%s %.2g" % kv for kv in rat.items()) + " of the bounds")
                    for nm, v in rat.items():
                        worst[nm] = max(worst.get(nm, 0.0), v)
    print("worst shares", worst)
    assert min(worst.values()) > 0 and worst["pred"] <= 0.01 and worst["dpred"] <= 0.01 and worst["var"] <= 0.1, worst


@pytest.mark.parametrize("extrapolate", (0, 1))
@pytest.mark.parametrize("K", pc.KS)
@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_against_the_yardstick(emu_model, pkg, problems, name, K, extrapolate):
    pb, ex = problems[name], extrapolate
    code, (got,), status = pc.call(pkg, emu_model, pb.k, K, ex, cov=pb.cov[K])
    assert code == 0, emu_model._lib.plh_last_error()
    assert (status == 0).all()
    for c in range(pb.k.n):
        pc.check_cell(pb, K, ex, c, pc.cell_of(got, c), pb.cov[K][c], name)
    if K == 1:                                           # one key, a positive 1 x 1 covariance: a variance that is negative would be a wrong formula, not cancellation
        assert (got["var"][:, ~np.isnan(pb.k.tq)] >= 0).all()


def test_one_two_and_three_channels(emu_model, pkg, problems):
    """channel i is another window of columns of the same field: its outputs have the same bits alone, with a second and with a third channel, in any position; an output
    whose pointer is NULL is left out and the others keep their bits; only the upper triangle of cov is read"""
    pb, K, ex = problems["main"], 3, 0
    k, firsts = pb.k, (0, 4, 5)
    cov = pb.cov[K]
    alone = []
    for f in firsts:
        code, (g,), _ = pc.call(pkg, emu_model, k, K, ex, cov=cov, chans=(f,))
        assert code == 0
        alone.append(g)
        for c in range(k.n):                             # (the covariance is that of columns 1 .. 3: for the other windows it is just a matrix, and the yardstick takes the same)
            pc.check_cell(pb, K, ex, c, pc.cell_of(g, c), cov[c], "channel at column %d" % f, first=f)
    code, two, _ = pc.call(pkg, emu_model, k, K, ex, cov=cov, chans=firsts[:2])
    assert code == 0 and pc.same_bits(two[0], alone[0]) and pc.same_bits(two[1], alone[1])
    code, three, status = pc.call(pkg, emu_model, k, K, ex, cov=cov, chans=(5, 0, 4))
    assert code == 0 and (status == 0).all()
    assert pc.same_bits(three[0], alone[2]) and pc.same_bits(three[1], alone[0]) and pc.same_bits(three[2], alone[1])
    # NULL outputs: every subset of a channel's three, differently per channel
    want = [("pred",), ("dpred", "var"), ("var",)]
    code, part, _ = pc.call(pkg, emu_model, k, K, ex, cov=cov, chans=firsts, want=want)
    assert code == 0
    for i in range(3):
        assert [nm for nm in pc.OUTS if part[i][nm] is not None] == list(want[i])
        assert pc.same_bits(part[i], alone[i], names=want[i])
    code, (nocov,), _ = pc.call(pkg, emu_model, k, K, ex, cov=None)                        # without a covariance: pred and dpred
    assert code == 0 and nocov["var"] is None and pc.same_bits(nocov, alone[0], names=("pred", "dpred"))
    junk = cov + np.tril(np.full((K, K), 1e30), -1)[None]                                 # the lower triangle is not read
    code, (g,), _ = pc.call(pkg, emu_model, k, K, ex, cov=junk)
    assert code == 0 and pc.same_bits(g, alone[0])


@pytest.mark.parametrize("K", (3, 8))
def test_held_and_unseen_keys(emu_model, pkg, problems, K):
    pb, ex = problems["main"], 0
    k = pb.k
    code, (full,), _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K])
    assert code == 0
    # held: 0 rows and columns -- the key contributes nothing: the variance of the problem without that key
    Mh = pc.held(pb.cov[K])
    code, (got,), _ = pc.call(pkg, emu_model, k, K, ex, cov=Mh)
    assert code == 0 and pc.same_bits(got, full, names=("pred", "dpred"))
    keep = [i for i in range(K) if i != pc.HELD]
    for c in range(k.n):
        pc.check_cell(pb, K, ex, c, pc.cell_of(got, c), Mh[c], "held key")
        ref = pc.reference(pb.S[ex][c], K, Mh[c])
        s = ref["dpred"][keep].astype(np.longdouble)
        without = (s * (Mh[c][np.ix_(keep, keep)].astype(np.longdouble) @ s)).sum(axis=0).astype(np.float64)
        rows = pc.compared(k, c, ex)
        assert np.array_equal(without[rows], ref["var"][rows])                             # (the yardstick agrees with itself: zeros add nothing)
        assert (np.abs(got["var"][c] - without)[rows] <= pc.bounds(k, c, K, ref, Mh[c])["var"][rows]).all()
    # unseen: NaN rows and columns -- var is NaN everywhere, pred and dpred keep their bits
    code, (got,), status = pc.call(pkg, emu_model, k, K, ex, cov=pc.unseen(pb.cov[K]))
    assert code == 0 and (status == 0).all()
    assert np.isnan(got["var"]).all() and pc.same_bits(got, full, names=("pred", "dpred"))
    # a failed covariance of ONE problem (all NaN): that cell's var only
    Mn = pb.cov[K].copy()
    Mn[1] = np.nan
    code, (got,), _ = pc.call(pkg, emu_model, k, K, ex, cov=Mn)
    assert code == 0 and np.isnan(got["var"][1]).all() and pc.same_bits(got, full, names=("pred", "dpred"))
    assert np.array_equal(got["var"][[0, 2]], full["var"][[0, 2]], equal_nan=True)


def test_nan_in_one_channels_sensitivities_stays_there(emu_model, pkg, problems):
    pb, K, ex = problems["main"], 3, 0
    k = pb.k
    code, clean, _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K], chans=(0, 4))
    assert code == 0
    cu, dc = pc.channel_arrays(k, K, 4)
    dc = dc.copy()
    dc[2, 1, :int(k.n_pts[2])] = np.nan                                                    # cell 2, key 1 of the second channel
    code, got, status = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K], chans=(0, 4), arrays={1: (cu, dc)})
    assert code == 0 and (status == 0).all()
    assert pc.same_bits(got[0], clean[0]) and pc.same_bits(got[1], clean[1], names=("pred",))
    fin = ~np.isnan(k.tq)
    assert np.isnan(got[1]["dpred"][2, 1]).all() and np.isnan(got[1]["var"][2]).all()
    for c in (0, 1):
        assert np.array_equal(got[1]["dpred"][c], clean[1]["dpred"][c], equal_nan=True) and np.array_equal(got[1]["var"][c], clean[1]["var"][c], equal_nan=True)
    assert np.array_equal(got[1]["dpred"][2, [0, 2]], clean[1]["dpred"][2, [0, 2]], equal_nan=True) and np.isfinite(got[1]["dpred"][2, 0, fin]).all()


def test_a_failed_cell_is_nan_and_its_neighbours_do_not_notice(emu_model, pkg, problems):
    pb, K, ex = problems["main"], 3, 0
    code, (clean,), _ = pc.call(pkg, emu_model, pb.k, K, ex, cov=pb.cov[K])
    assert code == 0
    k = copy.copy(pb.k)
    k.run_info = pb.k.run_info.copy()
    k.run_info[1, 1]["flag"] = -12                                                         # PLH_ERR_STALL in the second run of cell 1
    code, (got,), status = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K])
    assert code == 0 and list(status) == [0, 1, 0]
    for nm in pc.OUTS:
        assert np.isnan(got[nm][1]).all(), nm
        assert np.array_equal(got[nm][[0, 2]], clean[nm][[0, 2]], equal_nan=True), nm
    code, (got,), _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K], want_status=False)  # status may be NULL
    assert code == 0 and np.isnan(got["var"][1]).all() and np.array_equal(got["pred"][[0, 2]], clean["pred"][[0, 2]], equal_nan=True)


def test_a_nan_query_time_is_nan_there_and_nothing_else(emu_model, pkg, problems):
    pb, K, ex = problems["edge"], 8, 1
    k = pb.k
    code, (clean,), _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K])
    assert code == 0
    was = np.isnan(k.tq)
    assert was.sum() == 1 and all(np.isnan(clean[nm][..., was]).all() for nm in pc.OUTS)
    tq = k.tq.copy()
    tq[[3, 70]] = np.nan                                                                   # one in the first wave of queries, one in the second
    code, (got,), status = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K], tq=tq)
    assert code == 0 and (status == 0).all()
    now = np.isnan(tq)
    for nm in pc.OUTS:
        assert np.isnan(got[nm][..., now]).all() and np.array_equal(got[nm][..., ~now], clean[nm][..., ~now]), nm


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_a_query_at_a_saved_time_returns_the_saved_bits(emu_model, pkg, problems, name):
    pb, K = problems[name], 8
    k = pb.k
    curve, dcurve = pc.channel_arrays(k, K)
    for c in range(k.n):
        # every saved point but the first of a later run: that time is the join, which belongs to the run before
        rows = np.concatenate([np.arange(row + (1 if r else 0), row + m) for r, (row, m) in enumerate(k.runs[c])])
        tq = np.ascontiguousarray(k.t[c, rows])
        for ex in (0, 1):
            code, (got,), _ = pc.call(pkg, emu_model, k, K, ex, cells=[c], tq=tq)
            assert code == 0
            assert np.array_equal(got["pred"][0], curve[c, rows]) and np.array_equal(got["dpred"][0], dcurve[c][:, rows]), (name, c, ex)


def test_grouped_covariances(emu_model, pkg, problems):
    """3 cells in groups (2, 1): the members of a group use the group's matrix, and the bits are those of the per-cell call with the matrices repeated"""
    pb, K, ex = problems["main"], 8, 0
    k = pb.k
    G = pb.cov[K][[2, 0]]                                                                  # two matrices, neither of them cell 1's own
    code, (per_cell,), _ = pc.call(pkg, emu_model, k, K, ex, cov=G[[0, 0, 1]])
    assert code == 0
    code, (grouped,), status = pc.call(pkg, emu_model, k, K, ex, cov=G, group_off=[0, 2, 3], n_groups=2)
    assert code == 0 and (status == 0).all() and pc.same_bits(grouped, per_cell)
    code, (own,), _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K])
    fin = ~np.isnan(k.tq)
    assert not np.array_equal(own["var"][1, fin], grouped["var"][1, fin])                  # (the matrix matters)
    for c, g in ((0, 0), (1, 0), (2, 1)):
        pc.check_cell(pb, K, ex, c, pc.cell_of(grouped, c), G[g], "grouped")
    # one group of all cells, and one group per cell
    code, (one,), _ = pc.call(pkg, emu_model, k, K, ex, cov=G[:1], group_off=[0, 3], n_groups=1)
    code2, (rep,), _ = pc.call(pkg, emu_model, k, K, ex, cov=G[[0, 0, 0]])
    assert code == 0 and code2 == 0 and pc.same_bits(one, rep)
    code, (each,), _ = pc.call(pkg, emu_model, k, K, ex, cov=pb.cov[K], group_off=[0, 1, 2, 3], n_groups=3)
    assert code == 0 and pc.same_bits(each, own)


def test_invalid_arguments_write_nothing(emu_model, pkg, problems):
    pb, K = problems["main"], 3
    k, cov = pb.k, pb.cov[K]
    bad = [dict(raw=dict(n=0)), dict(raw=dict(n_runs=0)), dict(raw=dict(max_pts=0)), dict(raw=dict(n_q=0)), dict(raw=dict(n=-1)),
           dict(raw=dict(n_sens=0)), dict(raw=dict(n_sens=pkg._capi.LSQ_MAX_SENS + 1)), dict(raw=dict(n_ch=0)), dict(raw=dict(n_ch=4)),
           dict(raw=dict(extrapolate=2)), dict(raw=dict(extrapolate=-1)),
           dict(raw=dict(t=None)), dict(raw=dict(n_pts=None)), dict(raw=dict(run_info=None)), dict(raw=dict(ch=None)), dict(raw=dict(tq=None)),
           dict(raw={"ch0.curve": None}), dict(raw={"ch0.dcurve": None}), dict(chans=(0, 4), raw={"ch1.dcurve": None}),
           dict(want=[()]), dict(chans=(0, 4), want=[pc.OUTS, ()]),
           dict(raw=dict(cov=None)), dict(chans=(0, 4), want=[("pred",), ("var",)], raw=dict(cov=None)),
           dict(group_off=[0, 2, 3], n_groups=0), dict(group_off=[0, 1, 2, 3], n_groups=4), dict(group_off=[1, 2, 3], n_groups=2), dict(group_off=[0, 1, 2], n_groups=2),
           dict(group_off=[0, 2, 2, 3], n_groups=3), dict(group_off=[0, 3, 2, 3], n_groups=3)]
    for kw in bad:
        code, got, status = pc.call(pkg, emu_model, k, K, 0, cov=cov, **kw)
        assert code == pc.E_ARG, kw
        assert pc.untouched(got, status), kw
        assert b"plh_predict" in emu_model._lib.plh_last_error(), kw
    cap = pkg._capi
    ch = (cap.PredictChannel * 1)()
    assert emu_model._lib.plh_predict(emu_model._h, 1, 1, 1, None, None, None, 1, ch, 1, 1, None, 0, None, 0, None, None, 7, None) == pc.E_ARG        # an unknown ptr_kind
    code, _, _ = pc.call(pkg, emu_model, k, K, 0, cov=cov, chans=(0, 4), want=[("pred",), ("dpred",)], raw=dict(cov=None))                            # no var asked for: cov may be NULL
    assert code == 0


def _host_ensemble(pkg, model, k, K, chans=("V",)):
    """an EnsembleSolution over the synthetic case: V (I, T_avg) are windows of the field's columns, as the channels of predict_cases.call"""
    bufs = dict(t=k.t.copy(), n_pts=k.n_pts.copy(), run_info=k.run_info.copy(), SOC=None, Y=None, YP=None, counters=None, sens_keys=list(model.θ_keys[:K]))
    for name, first in zip(("V", "I", "T_avg"), (0, 4, 5)):
        cu, dc = pc.channel_arrays(k, K, first)
        bufs[name] = cu
        if name in chans:
            bufs[pkg.api.SENS_CHANNELS[name]] = dc
    return pkg.EnsembleSolution(model, bufs, ["I"] * k.n_runs)


def test_ensemble_predict_on_host_arrays(emu_model, pkg, problems):
    """EnsembleSolution.predict: the channels it evaluates, the covariance forms it takes, groups as labels or offsets, and what it refuses"""
    pb, K = problems["main"], 3
    k, cov = pb.k, pb.cov[K]
    ens = _host_ensemble(pkg, emu_model, k, K, chans=("V", "T_avg"))
    code, raw, raw_status = pc.call(pkg, emu_model, k, K, 0, cov=cov, chans=(0, 5))
    assert code == 0
    pr = ens.predict(k.tq, cov)
    assert isinstance(pr, pkg.EnsemblePrediction) and pr.channels == ["V", "T_avg"] and pr.keys == ens.keys and np.array_equal(pr.t, k.tq, equal_nan=True)
    for c, r in (("V", raw[0]), ("T_avg", raw[1])):
        got = dict(pred=getattr(pr, c), dpred=getattr(pr, "d%s_dtheta" % c), var=getattr(pr, c + "_var"))
        assert all(isinstance(v, np.ndarray) for v in got.values()) and pc.same_bits(got, r)
        assert got["pred"].shape == (k.n, len(k.tq)) and got["dpred"].shape == (k.n, K, len(k.tq))
        assert np.array_equal(getattr(pr, c + "_sd"), np.sqrt(np.maximum(r["var"], 0.0)), equal_nan=True)
    assert pr.I is None and pr.dI_dtheta is None and pr.I_var is None and pr.I_sd is None and np.array_equal(pr.status, raw_status)
    # a FitCovariance, one channel by name, extrapolation, no covariance
    fc = pkg.FitCovariance(ens.keys)
    fc.cov = cov
    one = ens.predict(k.tq, fc, channels="V", interp_bc="extrapolate")
    code, (rx,), _ = pc.call(pkg, emu_model, k, K, 1, cov=cov)
    assert one.channels == ["V"] and one.T_avg is None and np.array_equal(one.V_var, rx["var"], equal_nan=True) and np.array_equal(one.V, rx["pred"], equal_nan=True)
    bare = ens.predict(k.tq[:5])
    assert bare.V_var is None and bare.V_sd is None and np.array_equal(bare.dV_dtheta, raw[0]["dpred"][:, :, :5], equal_nan=True)
    assert ens.predict(float(k.tq[0])).V.shape == (k.n, 1)
    # a negative variance from cancellation is kept in var and clamped in sd only
    neg = ens.predict(k.tq, -cov, channels="V")
    fin = ~np.isnan(k.tq)
    assert (neg.V_var[:, fin] < 0).all() and (neg.V_sd[:, fin] == 0).all() and np.isnan(neg.V_sd[:, ~fin]).all()
    # groups: labels, or offsets
    G = cov[[2, 0]]
    code, (rg,), _ = pc.call(pkg, emu_model, k, K, 0, cov=G, group_off=[0, 2, 3], n_groups=2)
    for groups in ([0, 0, 1], np.array([0, 2, 3], np.int32)):
        assert np.array_equal(ens.predict(k.tq, G, groups=groups, channels="V").V_var, rg["var"], equal_nan=True)
    # refusals
    with pytest.raises(ValueError, match="sens"):
        _host_ensemble(pkg, emu_model, k, K, chans=()).predict(k.tq)                       # (sens_keys without a channel's sensitivities: no channel)
    with pytest.raises(ValueError, match="sensitivities of I"):
        ens.predict(k.tq, cov, channels=("V", "I"))
    with pytest.raises(ValueError, match="not one of"):
        ens.predict(k.tq, cov, channels="SOC")
    with pytest.raises(ValueError, match="cov must be"):
        ens.predict(k.tq, cov[:2])
    with pytest.raises(ValueError, match="cov must be"):
        ens.predict(k.tq, cov, groups=[0, 0, 1])
    with pytest.raises(ValueError, match="give cov"):
        ens.predict(k.tq, groups=[0, 0, 1])
    with pytest.raises(ValueError, match="groups"):
        ens.predict(k.tq, G, groups=[0, 2, 2])
    with pytest.raises(ValueError, match="interp_bc"):
        ens.predict(k.tq, cov, interp_bc="nearest")
    with pytest.raises(ValueError, match="1-D"):
        ens.predict(np.zeros((2, 2)), cov)
    plain = _host_ensemble(pkg, emu_model, k, K)
    plain.keys = []
    with pytest.raises(ValueError, match=r"sens=\[keys\]"):
        plain.predict(k.tq)
