"""plh_lsq_group and plh_group_scatter on the wave-emulator build of the device source (no GPU), host pointers, against the numpy restatement of the header's definition
(tests/lsq_group_cases.py: plain sequential loops).  The sums are compared bit for bit: the definition fixes the order of summation, and the inputs are made so that another
order shows."""
import numpy as np
import pytest

import lsq_group_cases as gc

N = int(np.sum(gc.SIZES))


def test_the_shape_is_the_one_intended():
    off = gc.offsets(gc.SIZES)
    assert N == 326 and off[0] == 0 and off[-1] == N and len(off) == 8
    assert np.array_equal(np.diff(off), gc.SIZES)


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_group_sums_have_the_bits_of_the_sequential_sum(emu_model, k):
    off = gc.offsets(gc.SIZES)
    cost, grad, JtJ = gc.make_fits(N, k, 10 + k)
    status = np.zeros(N, np.int32)
    cost[70] = np.nan                                                    # a member of group 3 (cells 66 .. 129)
    status[200] = 1                                                      # a member of group 5 (cells 195 .. 324), another group
    if k:
        grad[131, k - 1] = np.inf                                        # a member of group 4 (cells 130 .. 194)
    keep = [None if a is None else a.copy() for a in (cost, grad, JtJ, status, off)]
    ref = gc.sum_reference(off, cost, grad, JtJ, status)
    if k:
        # the test can tell orders of summation apart: numpy's pairwise sum over a group differs in bits from the sequential sum somewhere
        # (along the contiguous axis: that is where numpy sums pairwise)
        other = np.stack([np.sum(np.ascontiguousarray(grad[off[g]:off[g + 1]].T), axis=1) for g in range(len(gc.SIZES))])
        fin = np.isfinite(ref[1])
        assert (other[fin] != ref[1][fin]).any()
    out = gc.sum_outputs(len(gc.SIZES), k)
    rc = gc.call_sum(emu_model, off, cost, grad, JtJ, status, out)
    assert rc == 0, emu_model._lib.plh_last_error()
    assert gc.same_bits_nan(out["g_cost"], ref[0])
    if k:
        assert gc.same_bits_nan(out["g_grad"], ref[1]) and gc.same_bits_nan(out["g_JtJ"], ref[2])
    assert np.array_equal(out["g_status"], ref[3])
    # the NaN, the infinity and the status reach exactly their groups
    assert np.array_equal(np.isnan(out["g_cost"]), np.arange(7) == 3)
    assert np.array_equal(out["g_status"], (np.arange(7) == 5).astype(np.int32))
    if k:
        assert np.array_equal(~np.isfinite(out["g_grad"]).all(axis=1), np.arange(7) == 4)
        assert np.isfinite(out["g_JtJ"]).all()
    # groups of one have their member's bits
    for g, c in ((0, 0), (6, N - 1)):
        assert out["g_cost"][g].tobytes() == cost[c].tobytes()
        if k:
            assert out["g_grad"][g].tobytes() == grad[c].tobytes() and out["g_JtJ"][g].tobytes() == JtJ[c].tobytes()
    for a, b in zip((cost, grad, JtJ, status, off), keep):                # inputs unchanged
        assert a is None or a.tobytes() == b.tobytes()
    # a NULL status is 0 everywhere; a NULL g_status is allowed
    out2 = gc.sum_outputs(len(gc.SIZES), k, fill=7)
    assert gc.call_sum(emu_model, off, cost, grad, JtJ, None, out2) == 0
    assert (out2["g_status"] == 0).all() and gc.same_bits_nan(out2["g_cost"], ref[0])
    out3 = gc.sum_outputs(len(gc.SIZES), k, fill=7)
    assert gc.call_sum(emu_model, off, cost, grad, JtJ, status, out3, null=("g_status",)) == 0
    assert (out3["g_status"] == 7).all() and gc.same_bits_nan(out3["g_cost"], ref[0])


def test_one_group_and_one_group_per_cell(emu_model):
    k = 3
    cost, grad, JtJ = gc.make_fits(N, k, 31)
    status = (np.arange(N) % 50 == 7).astype(np.int32)
    for sizes in ([N], [1] * N):
        off = gc.offsets(sizes)
        ref = gc.sum_reference(off, cost, grad, JtJ, status)
        out = gc.sum_outputs(len(sizes), k)
        assert gc.call_sum(emu_model, off, cost, grad, JtJ, status, out) == 0, emu_model._lib.plh_last_error()
        for a, b in zip((out["g_cost"], out["g_grad"], out["g_JtJ"]), ref):
            assert gc.same_bits_nan(a, b)
        assert np.array_equal(out["g_status"], ref[3])
    assert out["g_cost"].tobytes() == cost.tobytes() and out["g_JtJ"].tobytes() == JtJ.tobytes() and np.array_equal(out["g_status"], status)


@pytest.mark.parametrize("k", [1, 8])
def test_scatter_writes_the_keys_of_the_members_and_nothing_else(emu_model, k):
    nth = 11
    off = gc.offsets(gc.SIZES)
    cols = np.array([9, 2, 10, 0, 5, 7, 1, 4][:k], np.int32)            # non-monotone
    theta = np.ascontiguousarray(1000.0 + np.arange(N * nth, dtype=np.float64).reshape(N, nth))          # distinct values
    g_theta = np.ascontiguousarray(-1.0 - np.arange(7 * nth, dtype=np.float64).reshape(7, nth))
    keep_g, theta0 = g_theta.copy(), theta.copy()
    assert gc.call_scatter(emu_model, off, cols, g_theta, theta) == 0, emu_model._lib.plh_last_error()
    lab = gc.labels(gc.SIZES)
    assert theta[:, cols].tobytes() == g_theta[lab][:, cols].tobytes()
    other = np.setdiff1d(np.arange(nth), cols)
    assert theta[:, other].tobytes() == theta0[:, other].tobytes()
    assert theta.tobytes() == gc.scatter_reference(off, cols, g_theta, theta0).tobytes()
    assert g_theta.tobytes() == keep_g.tobytes()


def test_refusals_write_nothing(emu_model):
    k, nth = 3, 11
    off = gc.offsets(gc.SIZES)
    cost, grad, JtJ = gc.make_fits(N, k, 77)
    status = np.zeros(N, np.int32)
    SENT = -777.0

    def refused_sum(what, off_=off, grad_=grad, JtJ_=JtJ, drop=(), **kw):
        out = gc.sum_outputs(len(off_) - 1 if "n_groups" not in kw else max(kw["n_groups"], 7), k, fill=SENT)
        for d in drop:
            out[d] = None
        rc = gc.call_sum(emu_model, off_, cost, grad_, JtJ_, status, out, **kw)
        assert rc == gc.E_ARG, (what, rc)
        for a in out.values():
            assert a is None or (a == SENT).all(), what

    bad = lambda i, v: np.ascontiguousarray(np.concatenate([off[:i], [v], off[i + 1:]]), dtype=np.int32)
    refused_sum("n_cells < 1", n_cells=0)
    refused_sum("n_groups < 1", n_groups=0)
    refused_sum("n_groups > n_cells", n_cells=5, n_groups=7)
    refused_sum("offsets do not start at 0", off_=bad(0, 1))
    refused_sum("offsets do not end at n_cells", off_=bad(7, N - 1))
    refused_sum("offsets past n_cells", off_=bad(7, N + 1))
    refused_sum("an empty group", off_=bad(3, 3))
    refused_sum("descending offsets", off_=bad(3, 1))
    refused_sum("n_sens < 0", n_sens=-1)
    refused_sum("n_sens > 8", n_sens=9)
    refused_sum("n_sens == 0 with grad", n_sens=0)
    refused_sum("n_sens > 0 without grad", null=("grad",))
    refused_sum("n_sens > 0 without JtJ", null=("JtJ",))
    refused_sum("n_sens > 0 without g_grad", drop=("g_grad",))
    refused_sum("n_sens > 0 without g_JtJ", drop=("g_JtJ",))
    refused_sum("no cost", null=("cost",))
    refused_sum("no g_cost", null=("g_cost",))
    refused_sum("no offsets", null=("group_off",))

    g_theta = np.full((7, nth), 5.0)

    def refused_scatter(what, cols=(9, 2, 10), off_=off, **kw):
        theta = np.full((N, nth), SENT)
        rc = gc.call_scatter(emu_model, off_, cols, g_theta, theta, **kw)
        assert rc == gc.E_ARG and (theta == SENT).all(), (what, rc)

    refused_scatter("n_cells < 1", n_cells=0)
    refused_scatter("n_groups < 1", n_groups=0)
    refused_scatter("n_groups > n_cells", n_cells=5, n_groups=7)
    refused_scatter("offsets do not start at 0", off_=bad(0, 1))
    refused_scatter("offsets do not end at n_cells", off_=bad(7, N - 1))
    refused_scatter("an empty group", off_=bad(3, 3))
    refused_scatter("n_keys < 1", n_keys=0)
    refused_scatter("n_keys > 8", cols=tuple(range(9)))
    refused_scatter("n_theta < 1", n_theta=0)
    refused_scatter("a column outside [0, n_theta)", cols=(9, 11))
    refused_scatter("a negative column", cols=(9, -1))
    refused_scatter("a column given twice", cols=(9, 2, 9))
    refused_scatter("no cols", null=("cols",))
    refused_scatter("no g_theta", null=("g_theta",))
    refused_scatter("no theta", null=("theta",))
    refused_scatter("no offsets", null=("group_off",))
