"""plh_lsq_multi: the least-squares objective over several measured channels in one pass (csrc/plh_lsq.h), on the wave-emulator build; the pointer-kind and chunking tests
again on the GPU (marked gpu).

Shapes: lsq_cases' "main" and "edge" cell-point sets (runs ending on, one past and one before a 64-point tile, a one-point run, the shortest spline), three cells, max_pts 140,
case width 3 (1 + K_MAX) = 27; channel c takes the columns 9 c .. 9 c + K of the case.
Yardstick: scipy (resample_cases.fitpack_reference), then lsq_cases.reference per channel, summed.  Every output is a sum over the channels, so the bound is the sum of
lsq_cases.bounds over the channels (each residual against its own channel's bound)."""
import copy

import numpy as np
import pytest

import lsq_cases as lc
import resample_cases as rc

NCH, CW = 3, 1 + lc.K_MAX
SHAPES = ((1, 8), (2, 0), (2, 1), (3, 3), (3, 8))            # (n_ch, K)


class Problem:
    """.k: the case at width 27; .S[ex] [cell, n_q, 27] by scipy; .Y[ch] [cell, n_q]; .W[ex][ch] [cell, n_q] (different per channel; 0 at the NaN query, and under
    extrapolate = 1 at the far queries of the cell)"""


def make_problem(pkg, name):
    p = Problem()
    p.k = k = rc.make_case(pkg, cell_points=lc.CASES[name], width=NCH * CW)
    p.S = {ex: rc.fitpack_reference(k, ex) for ex in (0, 1)}
    nq = len(k.tq)
    q = np.arange(nq)
    p.Y = [np.stack([p.S[0][(c + 1) % k.n, :, CW * ch] + 0.1 * np.cos(3.0 * q / nq + c + 0.7 * ch) for c in range(k.n)]) for ch in range(NCH)]
    p.W = {0: [], 1: []}
    for ch in range(NCH):
        base = 0.25 + 1.5 * np.random.default_rng(23 + ch).random(nq)
        base[np.isnan(k.tq)] = 0.0
        p.W[0].append(np.tile(base, (k.n, 1)))
        p.W[1].append(np.stack([np.where(rc.mild(k, c), base, 0.0) for c in range(k.n)]))
    return p


@pytest.fixture(scope="module")
def problems(pkg):
    return {name: make_problem(pkg, name) for name in lc.CASES}


def channel_case(k, ch):
    """the case as lsq_cases sees one channel: its nine columns"""
    kc = copy.copy(k)
    kc.src = k.src[:, :, CW * ch:CW * (ch + 1)]
    return kc


def channel_arrays(k, ch, K):
    return lc.arrays(channel_case(k, ch), K)


def summed_reference(pb, S, n_ch, K, ex, c, Y, W):
    """(reference, bound) of cell c: sums over the channels of lsq_cases.reference / lsq_cases.bounds; 'resid' a list per channel.  S: resampled values [cell, n_q, 27];
    Y[ch], W[ch]: this cell's rows"""
    ref, bnd = dict(cost=0.0, grad=np.zeros(K), JtJ=np.zeros((K, K)), resid=[]), dict(cost=0.0, grad=np.zeros(K), JtJ=np.zeros((K, K)), resid=[])
    for ch in range(n_ch):
        r = lc.reference(S[c][:, CW * ch:CW * ch + 1 + K], Y[ch], W[ch])
        b = lc.bounds(channel_case(pb.k, ch), c, K, lc.reference(pb.S[ex][c][:, CW * ch:CW * ch + 1 + K], Y[ch], W[ch]), W[ch])
        for nm in ("cost", "grad", "JtJ"):
            ref[nm] = ref[nm] + r[nm]; bnd[nm] = bnd[nm] + b[nm]
        ref["resid"].append(r["resid"]); bnd["resid"].append(b["resid"])
    return ref, bnd


def ratios(got, ref, bnd):
    out = {}
    for nm in ("cost", "grad", "JtJ"):
        if got.get(nm) is not None:
            out.update({nm: v for v in lc.ratios({nm: got[nm]}, ref, bnd).values()})
    for ch, r in enumerate(got["resid"]):
        if r is not None:
            out["resid%d" % ch] = lc.ratios(dict(resid=r), dict(resid=ref["resid"][ch]), dict(resid=bnd["resid"][ch]))["resid"]
    return out


def check_cell(pb, n_ch, K, ex, c, got, Y, W, label, S=None):
    ref, bnd = summed_reference(pb, pb.S[ex] if S is None else S, n_ch, K, ex, c, Y, W)
    rat = ratios(got, ref, bnd)
    print("%s n_ch %d K %d extrapolate %d cell %d: |got - ref| / bound " % (label, n_ch, K, ex, c) + " ".join("%s %.3g" % kv for kv in rat.items()))
    assert all(v <= 1.0 for v in rat.values()), (label, n_ch, K, ex, c, rat)


def call(pkg, p, k, n_ch, K, Y, W, per_cell, extrapolate, cells=None, tq=None, curves=None, dcurves=None, want_resid=True, want_status=True, kind=None, stream=None, dev=None,
         raw=None):
    """plh_lsq_multi on the case: channel ch = columns 9 ch .. 9 ch + K, data Y[ch] and weights W[ch] ([n_q], or [len(cells), n_q] with per_cell = 1; W[ch] may be None).
    Host pointers, or device tensors with kind = PLH_DEVICE.  raw: overrides of the call's arguments (the argument-error test).  Returns (rc, dict(cost, grad, JtJ, resid
    [per channel], status))"""
    cap = pkg._capi
    cells = list(range(k.n)) if cells is None else cells
    n = len(cells)
    tq = k.tq if tq is None else tq
    C_ = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    chans = []
    for ch in range(n_ch):
        V, dV = channel_arrays(k, ch, K)
        V = V if curves is None or curves[ch] is None else curves[ch]
        dV = dV if dcurves is None or dcurves[ch] is None else dcurves[ch]
        chans.append([C_(V[cells]), C_(dV[cells]) if K else None, C_(Y[ch]), C_(W[ch]), np.full((n, len(tq)), -777.0) if want_resid else None])
    ins = [np.ascontiguousarray(k.t[cells]), np.ascontiguousarray(k.n_pts[cells]), np.ascontiguousarray(k.run_info[cells])]
    outs = [np.full(n, -777.0), np.full((n, K), -777.0) if K else None, np.full((n, K, K), -777.0) if K else None, np.full(n, -7, np.int32)]
    if kind == cap.PLH_DEVICE:
        import torch
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to(dev)
        ins, outs, chans = [up(a) for a in ins], [up(a) for a in outs], [[up(a) for a in c] for c in chans]
        P = lambda a: None if a is None else a.data_ptr()
    else:
        kind = cap.PLH_HOST
        P = lambda a: None if a is None else a.ctypes.data
    arr = (cap.LsqChannel * max(n_ch, 1))()
    for ch in range(n_ch):
        arr[ch] = cap.LsqChannel(*[P(a) for a in chans[ch]])
    a = dict(n=n, n_runs=k.n_runs, max_pts=k.max_pts, t=P(ins[0]), n_pts=P(ins[1]), ri=P(ins[2]), n_ch=n_ch, ch=arr, n_sens=K, n_q=len(tq), tq=tq.ctypes.data, per_cell=per_cell,
             extrapolate=extrapolate, cost=P(outs[0]), grad=P(outs[1]), JtJ=P(outs[2]), status=P(outs[3]) if want_status else None, kind=kind, h=p._h)
    if raw:
        raw = dict(raw)
        for ch, member in raw.pop("null_member", ()):
            setattr(arr[ch], member, None)
        a.update(raw)
    code = p._lib.plh_lsq_multi(a["h"], a["n"], a["n_runs"], a["max_pts"], a["t"], a["n_pts"], a["ri"], a["n_ch"], a["ch"], a["n_sens"], a["n_q"], a["tq"], a["per_cell"],
                                a["extrapolate"], a["cost"], a["grad"], a["JtJ"], a["status"], a["kind"], stream)
    down = lambda x: None if x is None else x.cpu().numpy() if kind == cap.PLH_DEVICE else x
    if kind == cap.PLH_DEVICE:
        import torch
        torch.cuda.synchronize()
    return code, dict(cost=down(outs[0]), grad=down(outs[1]), JtJ=down(outs[2]), status=down(outs[3]), resid=[down(c[4]) for c in chans])


def cell_of(got, i):
    return {nm: (None if v is None else [None if r is None else r[i] for r in v] if nm == "resid" else v[i]) for nm, v in got.items()}


def same_bits(a, b, names=("cost", "grad", "JtJ", "resid")):
    eq = lambda x, y: (x is None and y is None) or np.array_equal(x, y, equal_nan=True)
    return all(all(eq(x, y) for x, y in zip(a[nm], b[nm])) and len(a[nm]) == len(b[nm]) if nm == "resid" else eq(a[nm], b[nm]) for nm in names)


def rows(A, n_ch, c=None):
    return [A[ch] if c is None else A[ch][c] for ch in range(n_ch)]


def test_restatement_sits_far_inside_the_summed_bounds(problems):
    """the numpy restatement of the resample algorithm, summed over three channels the same way, sits inside RESTATEMENT_SHARE of the summed bounds (no code under test)"""
    worst = {}
    for name, pb in problems.items():
        for ex in (0, 1):
            mine = rc.restatement(pb.k, ex)
            for c in range(pb.k.n):
                Y, W = rows(pb.Y, NCH, c), rows(pb.W[ex], NCH, c)
                ref, bnd = summed_reference(pb, pb.S[ex], NCH, lc.K_MAX, ex, c, Y, W)
                got, _ = summed_reference(pb, mine, NCH, lc.K_MAX, ex, c, Y, W)
                rat = ratios(got, ref, bnd)
                print("%s extrapolate %d cell %d: restatement at " % (name, ex, c) + " ".join("%s %.2g" % kv for kv in rat.items()) + " of the summed bounds")
                for nm, v in rat.items():
                    worst[nm] = max(worst.get(nm, 0.0), v)
    assert max(worst.values()) > 0 and all(v <= lc.RESTATEMENT_SHARE for v in worst.values()), worst


@pytest.mark.parametrize("extrapolate", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "ch%d-K%d" % s)
@pytest.mark.parametrize("name", tuple(lc.CASES))
def test_against_the_yardstick(emu_model, pkg, problems, name, shape, extrapolate):
    pb, ex, (n_ch, K) = problems[name], extrapolate, shape
    k = pb.k
    code, got = call(pkg, emu_model, k, n_ch, K, rows(pb.Y, n_ch), rows(pb.W[ex], n_ch), 1, ex)          # every cell with its own data and weights
    assert code == 0, emu_model._lib.plh_last_error()
    assert (got["status"] == 0).all()
    if K:
        assert np.array_equal(got["JtJ"], got["JtJ"].transpose(0, 2, 1))
    else:
        assert got["grad"] is None and got["JtJ"] is None
    for c in range(k.n):
        Y, W = rows(pb.Y, n_ch, c), rows(pb.W[ex], n_ch, c)
        check_cell(pb, n_ch, K, ex, c, cell_of(got, c), Y, W, "per-cell data")
        for ch in range(n_ch):
            assert (got["resid"][ch][c][W[ch] == 0] == 0).all()
        code, one = call(pkg, emu_model, k, n_ch, K, Y, W, 0, ex, cells=[c])                                # shared data, cell by cell: the same bits
        assert code == 0 and one["status"].tolist() == [0]
        assert same_bits(cell_of(one, 0), cell_of(got, c))
    if n_ch == 1:                                                                                          # one channel: plh_lsq's bits
        code, single = lc.call(pkg, emu_model, k, K, pb.Y[0], pb.W[ex][0], 1, ex)
        assert code == 0
        assert all(single[nm] is None and got[nm] is None or np.array_equal(single[nm], got[nm], equal_nan=True) for nm in ("cost", "grad", "JtJ"))
        assert np.array_equal(single["resid"], got["resid"][0], equal_nan=True)


def test_one_channel_is_plh_lsq_bit_for_bit(emu_model, pkg, problems):
    """every K of plh_lsq's own suite, and any of the three column groups as the one channel"""
    for name, pb in problems.items():
        for K in lc.KS:
            code, single = lc.call(pkg, emu_model, pb.k, K, pb.Y[0], pb.W[1][0], 1, 1)
            code2, got = call(pkg, emu_model, pb.k, 1, K, [pb.Y[0]], [pb.W[1][0]], 1, 1)
            assert code == 0 and code2 == 0
            assert all(single[nm] is None and got[nm] is None or np.array_equal(single[nm], got[nm], equal_nan=True) for nm in ("cost", "grad", "JtJ"))
            assert np.array_equal(single["resid"], got["resid"][0], equal_nan=True) and np.array_equal(single["status"], got["status"])


@pytest.mark.parametrize("name", tuple(lc.CASES))
def test_a_channel_with_null_weights(emu_model, pkg, problems, name):
    pb, n_ch, K = problems[name], 3, 3
    k = pb.k
    keep = ~np.isnan(k.tq)
    tq = np.ascontiguousarray(k.tq[keep])
    Y = [np.ascontiguousarray(y[:, keep]) for y in pb.Y]
    W = [np.ascontiguousarray(w[:, keep]) for w in pb.W[0]]
    W[1] = None
    code, got = call(pkg, emu_model, k, n_ch, K, Y, W, 1, 0, tq=tq)
    assert code == 0
    ones = [W[0], np.ones_like(Y[1]), W[2]]
    code, ref1 = call(pkg, emu_model, k, n_ch, K, Y, ones, 1, 0, tq=tq)
    assert code == 0 and same_bits(got, ref1)
    S = pb.S[0][:, keep]
    sub = copy.copy(pb)
    sub.S = {0: S}
    for c in range(k.n):
        check_cell(sub, n_ch, K, 0, c, cell_of(got, c), rows(Y, n_ch, c), rows(ones, n_ch, c), "w = NULL in channel 1")
    # shared data with the NULL channel: the same bits cell by cell
    code, one = call(pkg, emu_model, k, n_ch, K, rows(Y, n_ch, 2), [W[0][2], None, W[2][2]], 0, 0, tq=tq, cells=[2])
    assert code == 0 and same_bits(cell_of(one, 0), cell_of(got, 2))


def test_a_point_left_out_of_one_channel_still_counts_in_the_others(emu_model, pkg, problems):
    pb, n_ch, K = problems["main"], 3, 3
    k = pb.k
    finite = np.nonzero(~np.isnan(k.tq))[0]
    out = finite[[2, 40, 66]]
    W = [w.copy() for w in pb.W[0]]
    W[1][:, out] = 0.0
    code, base = call(pkg, emu_model, k, n_ch, K, pb.Y, W, 1, 0)
    assert code == 0 and (base["resid"][1][:, out] == 0).all() and np.isfinite(base["cost"]).all()
    assert (base["resid"][0][:, out] != 0).all() and (base["resid"][2][:, out] != 0).all()                 # the other channels count that time
    Y = [y.copy() for y in pb.Y]
    Y[1][:, out] = np.nan                                                                                  # a NaN datum where the channel has weight 0: no bit changes
    code, got = call(pkg, emu_model, k, n_ch, K, Y, W, 1, 0)
    assert code == 0 and same_bits(got, base)
    for c in range(k.n):
        check_cell(pb, n_ch, K, 0, c, cell_of(got, c), rows(pb.Y, n_ch, c), rows(W, n_ch, c), "w = 0 in channel 1")
    # the same datum weighed: cost, grad and that residual of that cell are NaN; JtJ does not hold the data; the other cells do not notice
    W2 = [w.copy() for w in W]
    W2[1][1, out[0]] = 0.7
    code, got = call(pkg, emu_model, k, n_ch, K, Y, W2, 1, 0)
    assert code == 0 and np.isnan(got["cost"][1]) and np.isnan(got["grad"][1]).all() and np.isfinite(got["JtJ"][1]).all()
    assert np.isnan(got["resid"][1][1, out[0]]) and np.isfinite(got["resid"][0][1][W2[0][1] != 0]).all()
    assert same_bits(cell_of(got, 0), cell_of(base, 0)) and same_bits(cell_of(got, 2), cell_of(base, 2))


def test_failed_cell_is_nan_and_its_neighbours_do_not_notice(emu_model, pkg, problems):
    pb, n_ch, K = problems["main"], 3, 3
    k = pb.k
    code, whole = call(pkg, emu_model, k, n_ch, K, pb.Y, pb.W[0], 1, 0)
    assert code == 0
    bad = copy.copy(k)
    bad.run_info = k.run_info.copy()
    bad.run_info[1, 1]["flag"] = pkg._capi.ERR_STALL
    bad.src = k.src.copy()
    bad.src[1] = np.nan                                                                                    # (none of its points is read)
    code, got = call(pkg, emu_model, bad, n_ch, K, pb.Y, pb.W[0], 1, 0)
    assert code == 0 and got["status"].tolist() == [0, 1, 0]
    assert all(np.isnan(got[nm][1]).all() for nm in ("cost", "grad", "JtJ")) and all(np.isnan(r[1]).all() for r in got["resid"])
    for c in (0, 2):
        assert same_bits(cell_of(got, c), cell_of(whole, c))


def test_nan_sensitivities_of_one_channel_stay_in_their_cell(emu_model, pkg, problems):
    pb, n_ch, K = problems["main"], 3, 3
    k = pb.k
    code, whole = call(pkg, emu_model, k, n_ch, K, pb.Y, pb.W[0], 1, 0)
    _, dV = channel_arrays(k, 1, K)
    dV[2, 1, :int(k.n_pts[2])] = np.nan                                                                    # one row of one cell of channel 1
    code, got = call(pkg, emu_model, k, n_ch, K, pb.Y, pb.W[0], 1, 0, dcurves=[None, dV, None])
    assert code == 0 and (got["status"] == 0).all()
    assert np.isnan(got["grad"][2, 1]) and np.isnan(got["JtJ"][2, 1, :]).all() and np.isnan(got["JtJ"][2, :, 1]).all()
    keep = [0, 2]
    assert np.array_equal(got["grad"][2, keep], whole["grad"][2, keep]) and np.array_equal(got["JtJ"][2][np.ix_(keep, keep)], whole["JtJ"][2][np.ix_(keep, keep)])
    assert same_bits(cell_of(got, 2), cell_of(whole, 2), names=("cost", "resid"))
    for c in (0, 1):
        assert same_bits(cell_of(got, c), cell_of(whole, c))


def test_argument_errors(emu_model, pkg, problems):
    pb, n_ch, K = problems["main"], 2, 2
    k, cap = pb.k, pkg._capi
    Y, W = [pb.Y[0][0], pb.Y[1][0]], [pb.W[0][0][0], pb.W[0][1][0]]
    go = lambda **raw: call(pkg, emu_model, k, n_ch, K, Y, W, 0, 0, raw=raw)
    code, ok = go()
    assert code == 0 and (ok["cost"] != -777.0).all()
    for raw in (dict(n=0), dict(n_runs=0), dict(max_pts=0), dict(n_q=0), dict(n_q=-2), dict(n_sens=-1), dict(n_sens=cap.LSQ_MAX_SENS + 1), dict(per_cell=2), dict(per_cell=-1),
                dict(extrapolate=2), dict(t=None), dict(n_pts=None), dict(ri=None), dict(tq=None), dict(cost=None), dict(grad=None), dict(JtJ=None), dict(n_sens=0),
                dict(n_sens=0, grad=None), dict(kind=cap.PLH_HOST_ASYNC), dict(h=None),
                dict(n_ch=0), dict(n_ch=-1), dict(n_ch=cap.LSQ_MAX_CHANNELS + 1), dict(ch=None),
                dict(null_member=[(0, "curve")]), dict(null_member=[(1, "curve")]), dict(null_member=[(1, "y")]), dict(null_member=[(1, "dcurve")]),
                dict(n_sens=0, grad=None, JtJ=None), dict(n_sens=0, grad=None, JtJ=None, null_member=[(0, "dcurve")])):
        code, got = go(**raw)
        assert code == rc.E_ARG, raw
        assert emu_model._lib.plh_last_error()
        assert (got["cost"] == -777.0).all() and all((r == -777.0).all() for r in got["resid"]) and (got["status"] == -7).all(), raw       # refused before anything ran
    code, got = go(n_sens=0, grad=None, JtJ=None, null_member=[(0, "dcurve"), (1, "dcurve")])              # the misfit-only call
    assert code == 0 and np.array_equal(got["cost"], ok["cost"])
    code, got = go(null_member=[(0, "w"), (1, "resid")])                                                  # w and resid may be NULL
    assert code == 0


def chunk_case(pkg, pts):
    K = 8
    k = rc.make_case(pkg, cell_points=pts, width=NCH * CW, seed=5)
    rng = np.random.default_rng(1)
    Y = [4.0 + rng.random((k.n, len(k.tq))) for _ in range(NCH)]
    W = [np.where(np.isnan(k.tq), 0.0, 0.5 + rng.random((k.n, len(k.tq)))) for _ in range(NCH)]
    return k, K, Y, W


def test_chunked_workspace_gives_the_same_bits(emu_model, pkg, monkeypatch):
    k, K, Y, W = chunk_case(pkg, ((5, 9), (1, 2), (70, 3), (4, 4), (2, 30)))
    code, whole = call(pkg, emu_model, k, NCH, K, Y, W, 1, 0)
    assert code == 0 and (whole["status"] == 0).all() and np.isfinite(whole["JtJ"]).all()
    for budget in (1, 2 * 8 * k.max_pts * NCH * CW + 8192):                                               # one cell per chunk, then two
        monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(budget))
        code, got = call(pkg, emu_model, k, NCH, K, Y, W, 1, 0)
        assert code == 0 and (got["status"] == 0).all() and same_bits(got, whole), budget


@pytest.mark.gpu
def test_chunked_workspace_gives_the_same_bits_gpu(hip_model, pkg, monkeypatch):
    import torch
    cap = pkg._capi
    k, K, Y, W = chunk_case(pkg, ((5, 9), (1, 2), (70, 3), (4, 4), (2, 30), (7, 100), (3, 3), (64, 64), (2, 2)))
    stream = torch.cuda.Stream()
    code, whole = call(pkg, hip_model, k, NCH, K, Y, W, 1, 0, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and (whole["status"] == 0).all() and np.isfinite(whole["JtJ"]).all()
    monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", "1")                                                      # one cell per chunk
    code, got = call(pkg, hip_model, k, NCH, K, Y, W, 1, 0, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
    assert code == 0 and same_bits(got, whole)
    code, got = call(pkg, hip_model, k, NCH, K, Y, W, 1, 0)                                                # and through host pointers
    assert code == 0 and same_bits(got, whole)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((3, 8), (2, 0), (1, 8)), ids=lambda s: "ch%d-K%d" % s)
def test_device_pointers_on_a_stream_equal_host_pointers_gpu(hip_model, pkg, problems, shape):
    import torch
    cap, (n_ch, K) = pkg._capi, shape
    stream = torch.cuda.Stream()
    for name, pb in problems.items():
        k = pb.k
        for ex in (0, 1):
            Y, W = rows(pb.Y, n_ch), rows(pb.W[ex], n_ch)
            code, host = call(pkg, hip_model, k, n_ch, K, Y, W, 1, ex)
            assert code == 0, hip_model._lib.plh_last_error()
            code, dev = call(pkg, hip_model, k, n_ch, K, Y, W, 1, ex, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
            assert code == 0, hip_model._lib.plh_last_error()
            assert same_bits(host, dev) and (host["status"] == 0).all() and (dev["status"] == 0).all()
            for c in range(k.n):
                check_cell(pb, n_ch, K, ex, c, cell_of(dev, c), rows(pb.Y, n_ch, c), rows(pb.W[ex], n_ch, c), "device pointers")
            if n_ch == 1:
                code, single = lc.call(pkg, hip_model, k, K, pb.Y[0], pb.W[ex][0], 1, ex, kind=cap.PLH_DEVICE, stream=stream.cuda_stream, dev="cuda")
                assert code == 0 and all(np.array_equal(single[nm], dev[nm], equal_nan=True) for nm in ("cost", "grad", "JtJ")) and np.array_equal(single["resid"], dev["resid"][0], equal_nan=True)
