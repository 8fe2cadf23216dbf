"""Selected state sections per saved point on the GPU (plh_outputs.sel / Y_sel, `sections=`): the ensembles of the benchmark configurations keep the named sections only,
packed, in HBM -- and those are the bits of the corresponding columns of the full state dump (outputs = "all"), with every other output unchanged (the two calls run the same
kernel instantiation).  tests/test_selected_outputs.py holds the argument rules, truncation and the single-cell API on the emulator build."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(x):
    import torch
    return x.contiguous().view(torch.int64)


def check_against_full_dump(pkg, p, cfg, n, n_full, sections):
    """n cells with sections= and the first n_full of them with outputs = "all", both device-resident"""
    import torch
    Thd = torch.from_numpy(np.ascontiguousarray(cfg["theta"])).cuda()
    mp = cfg["max_points"]
    ens = pkg.simulate_ensemble(p, Thd, cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=mp, sections=sections)
    torch.cuda.synchronize()
    kms = ens.kernel_ms
    lens = [p.ind[s].stop - p.ind[s].start for s in sections]
    assert ens.Y_all is None and ens.Y_sel.is_cuda and tuple(ens.Y_sel.shape) == (n, mp, sum(lens))
    assert ens.Y_sel.numel() * ens.Y_sel.element_size() == n * mp * sum(lens) * 8                      # the allocation: cells x max_points x selected entries x 8 bytes
    full = pkg.simulate_ensemble(p, Thd[:n_full], cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=mp, outputs="all")
    torch.cuda.synchronize()
    assert full.Y_sel is None and tuple(full.Y_all.shape) == (n_full, mp, p.N.tot)
    npts = full.n_pts.to(torch.int64)
    assert torch.equal(ens.n_pts[:n_full], full.n_pts) and int(npts.min()) >= 1 and int(npts.max()) <= mp
    valid = torch.arange(mp, device=npts.device)[None, :] < npts[:, None]                              # [cell, point]: the saved points
    off = 0
    for s, ln in zip(sections, lens):
        assert ens.sel_ind[s] == slice(off, off + ln)
        a, b = ens.Y_sel[:n_full, :, off:off + ln][valid], full.Y_all[:, :, p.ind[s]][valid]
        assert a.shape == (int(npts.sum()), ln) and torch.equal(bits(a), bits(b)), s
        assert torch.equal(bits(ens.section(s)[:n_full][valid]), bits(b)), s
        off += ln
    for nm in ("t", "V", "I", "SOC") + (("T_avg",) if p.temperature else ()):
        assert torch.equal(bits(getattr(ens, nm)[:n_full][valid]), bits(getattr(full, nm)[valid])), nm
    assert torch.equal(bits(ens.Y[:n_full]), bits(full.Y)) and torch.equal(bits(ens.YP[:n_full]), bits(full.YP))
    assert ens.run_info[:n_full].tobytes() == full.run_info.tobytes() and ens.counters[:n_full].tobytes() == full.counters.tobytes()
    print("%s, %d cells, sections %s: kernel %.3f ms, Y_sel %.1f MB (the full dump of the same cells would be %.1f MB)"
          % (cfg["name"], n, sections, kms, ens.Y_sel.numel() * 8 / 1e6, n * mp * p.N.tot * 8 / 1e6))
    return ens


def test_c4_shard_keeps_c_e_only(pkg, hip_model):
    p = hip_model
    ens = check_against_full_dump(pkg, p, pkg.configs.c4(p, 8192), 8192, 1024, ("c_e",))
    assert ens.Y_sel.numel() * 8 == 8192 * 256 * 30 * 8


def test_c5_film_and_soh(pkg, hip_model_nmc_sei):
    p = hip_model_nmc_sei
    check_against_full_dump(pkg, p, pkg.configs.c5(p, 256), 256, 256, ("film", "SOH"))


def test_c3_temperature_and_c_e(pkg, hip_model_thermal):
    p = hip_model_thermal
    check_against_full_dump(pkg, p, pkg.configs.c3(p, 256), 256, 256, ("T", "c_e"))


def test_three_host_paths_agree(pkg, hip_model_thermal):
    """blocking PLH_HOST with fresh arrays, PLH_HOST_ASYNC through HostPipeline, PLH_DEVICE: the same bits in Y_sel (and in t, V, n_pts)"""
    import torch
    p = hip_model_thermal
    n = 256
    cfg = pkg.configs.c3(p, n)
    Th = np.ascontiguousarray(cfg["theta"])
    sections = ("T", "c_e")
    e = pkg.simulate_ensemble(p, torch.from_numpy(Th).cuda(), cfg["protocol"], SOC=cfg["SOC"], device=True, max_points=cfg["max_points"], sections=sections)
    torch.cuda.synchronize()
    h = pkg.simulate_ensemble(p, Th, cfg["protocol"], SOC=cfg["SOC"], max_points=cfg["max_points"], sections=sections)
    pipe = pkg.api.HostPipeline(p, n, cfg["protocol"], SOC=cfg["SOC"], max_points=cfg["max_points"], sections=sections)
    try:
        pipe.submit(0, Th)
        pipe.submit(1, Th)
        slots = [{k: np.array(v) for k, v in pipe.wait(s).items() if k in ("t", "V", "n_pts", "Y_sel")} for s in (0, 1)]
        assert pipe.sel_ind == h.sel_ind == e.sel_ind
    finally:
        pipe.close()
    npd = e.n_pts.cpu().numpy()
    ed = {k: getattr(e, k).cpu().numpy() for k in ("t", "V", "Y_sel")}
    assert h.Y_all is None and isinstance(h.Y_sel, np.ndarray) and h.Y_sel.shape == ed["Y_sel"].shape == (n, cfg["max_points"], 80)
    assert np.array_equal(h.n_pts, npd) and all(np.array_equal(s["n_pts"], npd) for s in slots) and npd.min() >= 1
    for i in range(n):
        k = int(npd[i])
        for nm in ("t", "V", "Y_sel"):
            assert np.array_equal(np.asarray(getattr(h, nm))[i, :k], ed[nm][i, :k]), ("PLH_HOST", nm, i)
            for q, s in enumerate(slots):
                assert np.array_equal(s[nm][i, :k], ed[nm][i, :k]), ("PLH_HOST_ASYNC slot %d" % q, nm, i)
    assert np.array_equal(np.asarray(h.T_avg)[0, :int(npd[0])], e.T_avg.cpu().numpy()[0, :int(npd[0])])


OPTIONAL = ("t", "V", "I", "SOC", "T_avg", "n_pts", "Y_final", "YP_final", "counters", "Y_all", "Y_sel")
PER_POINT = ("t", "V", "I", "SOC", "T_avg", "Y_all", "Y_sel")


def _three_kinds(pkg, p, Th, proto, soc, mp, want, sel):
    """one plh_integrate per pointer kind with the arrays of `want` (+ run_info): PLH_DEVICE on torch tensors, a blocking PLH_HOST call with fresh numpy arrays, PLH_HOST_ASYNC
    through a one-slot HostPipeline whose slot carries pinned arrays for exactly these outputs -> three {name: numpy array}"""
    import ctypes as C
    import torch
    cap, lib = pkg._capi, p._lib
    n, N = Th.shape[0], p.N.tot
    sel_arr = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1, 2)
    runs, _ = pkg.make_protocol(p, proto, n)
    shapes = dict(t=((n, mp), np.float64), V=((n, mp), np.float64), I=((n, mp), np.float64), SOC=((n, mp), np.float64), T_avg=((n, mp), np.float64),
                  n_pts=((n,), np.int32), Y_final=((n, N), np.float64), YP_final=((n, N), np.float64), run_info=((n, len(runs)), cap.RUN_INFO_DTYPE),
                  counters=((n,), cap.COUNTERS_DTYPE), Y_all=((n, mp, N), np.float64), Y_sel=((n, mp, int(sel_arr[:, 1].sum())), np.float64))
    names = tuple(want) + ("run_info",)
    nbytes = lambda nm: int(np.prod(shapes[nm][0])) * np.dtype(shapes[nm][1]).itemsize

    def outputs(b):
        out = cap.Outputs()
        out.max_pts = mp
        for nm in names:
            setattr(out, nm, cap.ptr(b[nm]))
        out.n_sel, out.sel = len(sel_arr), sel_arr.ctypes.data_as(C.POINTER(C.c_int))
        return out
    view = lambda raw, nm: raw.view(shapes[nm][1]).reshape(shapes[nm][0])
    opts = pkg.api._opts_struct(p.opts, p)
    arr = (cap.Run * len(runs))(*runs)
    res = {}
    # PLH_DEVICE
    dev = {nm: torch.empty(nbytes(nm), dtype=torch.uint8, device="cuda") for nm in names}
    Thd, socd = torch.from_numpy(Th).cuda(), torch.full((n,), float(soc), dtype=torch.float64, device="cuda")
    out = outputs(dev)
    cap.check(lib, lib.plh_integrate(p._h, n, cap.ptr(Thd), cap.ptr(socd), None, None, len(runs), arr, C.byref(opts), C.byref(out), cap.PLH_DEVICE, None), "PLH_DEVICE")
    torch.cuda.synchronize()
    res["PLH_DEVICE"] = {nm: view(dev[nm].cpu().numpy(), nm) for nm in names}
    # PLH_HOST, arrays no one has touched
    host = {nm: np.empty(nbytes(nm), np.uint8) for nm in names}
    out, soch = outputs(host), np.full(n, float(soc))
    cap.check(lib, lib.plh_integrate(p._h, n, cap.ptr(Th), cap.ptr(soch), None, None, len(runs), arr, C.byref(opts), C.byref(out), cap.PLH_HOST, None), "PLH_HOST")
    res["PLH_HOST"] = {nm: view(host[nm], nm) for nm in names}
    # PLH_HOST_ASYNC
    pipe = pkg.api.HostPipeline(p, n, proto, SOC=soc, max_points=mp, depth=1)
    try:
        pin = {}
        for nm in names:
            ptr = C.c_void_p()
            cap.check(lib, lib.plh_host_alloc(C.byref(ptr), nbytes(nm)), "plh_host_alloc")
            pipe._blocks.append(ptr)                                       # (freed by pipe.close() with the pipeline's own)
            pin[nm] = np.frombuffer((C.c_char * nbytes(nm)).from_address(ptr.value), dtype=np.uint8)
        pipe.slots[0]["out"] = outputs(pin)
        pipe.submit(0, Th)
        pipe.wait(0)
        res["PLH_HOST_ASYNC"] = {nm: view(pin[nm].copy(), nm) for nm in names}
    finally:
        pipe.close()
    return res


def _same_bits(res, want, n_pts, what):
    ref = res["PLH_DEVICE"]
    for kind in ("PLH_HOST", "PLH_HOST_ASYNC"):
        got = res[kind]
        assert got["run_info"].tobytes() == ref["run_info"].tobytes(), (what, kind)
        for nm in want:
            if nm in PER_POINT:
                for c in range(len(n_pts)):
                    k = int(n_pts[c])
                    assert got[nm][c, :k].tobytes() == ref[nm][c, :k].tobytes(), (what, kind, nm, c)
            else:
                assert got[nm].tobytes() == ref[nm].tobytes(), (what, kind, nm)


@pytest.mark.parametrize("variant", ["lco_iso", "lco_thermal"])
def test_output_subsets_agree_across_pointer_kinds(pkg, hip_model, hip_model_thermal, variant):
    """every requested array holds the same bits whichever way it travels -- everything, run_info alone, everything but n_pts (which the way back of a blocking host call
    then keeps on the device for itself); 5 cells that differ, 64 points"""
    p = hip_model if variant == "lco_iso" else hip_model_thermal
    n, mp = 5, 64
    Th = np.ascontiguousarray(pkg.configs.sweep_theta(p, np.arange(n), 4))
    proto = [{"I": -1.0, "tf": 1200.0}]
    sel = [(p.ind["Φ_e"].start + 3, 7), (p.ind["c_e"].start + 2, 5)]
    n_pts = None
    for name, want in (("everything", OPTIONAL), ("only run_info", ()), ("no n_pts", tuple(k for k in OPTIONAL if k != "n_pts"))):
        res = _three_kinds(pkg, p, Th, proto, 1.0, mp, want, sel)
        if n_pts is None:
            n_pts = res["PLH_DEVICE"]["n_pts"].copy()
            assert 8 <= n_pts.min() and n_pts.max() <= mp and len(set(n_pts.tolist())) > 1, n_pts
            assert (res["PLH_DEVICE"]["run_info"]["flag"] == 0).all()
        _same_bits(res, want, n_pts, (variant, name))


def test_large_output_block_agrees_across_pointer_kinds(pkg, hip_model):
    """600 cells with every saved state vector: the output block is far beyond the size at which the way back of a blocking host call starts its team of copying threads
    and cuts Y_all into pieces (92 MB)"""
    p = hip_model
    n, mp = 600, 64
    Th = np.ascontiguousarray(pkg.configs.sweep_theta(p, np.arange(n), 4))
    want = ("t", "V", "I", "SOC", "n_pts", "Y_final", "YP_final", "counters", "Y_all")
    res = _three_kinds(pkg, p, Th, [{"I": -1.0, "tf": 1200.0}], 1.0, mp, want, [(0, 1)])
    n_pts = res["PLH_DEVICE"]["n_pts"]
    assert 8 <= n_pts.min() and n_pts.max() <= mp
    _same_bits(res, want, n_pts, "600 cells, outputs = all")


def test_names_follow_the_grid(pkg, hip_model):
    """p.ind of a registered grid library differs from the default grid's: the name -> range mapping of sections= follows the model it is given"""
    import torch
    p12 = pkg.petlion(pkg.LCO, N_p=12, N_s=7, N_n=9, N_r_p=11, N_r_n=11)
    assert p12.ind["c_e"] != hip_model.ind["c_e"] or p12.ind["Φ_s"] != hip_model.ind["Φ_s"]
    assert p12.ind["c_e"].stop - p12.ind["c_e"].start == 28 and p12.ind["Φ_s"].start != hip_model.ind["Φ_s"].start
    n = 64
    for p in (hip_model, p12):
        Th = torch.from_numpy(pkg.configs.sweep_theta(p, np.arange(n), 4)).cuda()
        proto = [{"I": -1.0, "tf": 900.0}, {"I": 1.0, "tf": 600.0, "V_max": 4.0}]
        sections = ("Φ_s", "j", "c_e")
        ens = pkg.simulate_ensemble(p, Th, proto, SOC=0.9, device=True, max_points=256, sections=sections)
        full = pkg.simulate_ensemble(p, Th, proto, SOC=0.9, device=True, max_points=256, outputs="all")
        torch.cuda.synchronize()
        assert ens.sel == tuple((p.ind[s].start, p.ind[s].stop - p.ind[s].start) for s in sections)
        assert torch.equal(ens.n_pts, full.n_pts) and ens.run_info.tobytes() == full.run_info.tobytes()
        valid = torch.arange(256, device=Th.device)[None, :] < full.n_pts.to(torch.int64)[:, None]
        for s in sections:
            assert torch.equal(bits(ens.section(s)[valid]), bits(full.Y_all[:, :, p.ind[s]][valid])), (p.N.tot, s)
        # the terminal voltage from the selected Φ_s is the V the kernel saved
        ps = ens.section("Φ_s")
        assert torch.equal(bits((ps[:, :, 0] - ps[:, :, -1])[valid]), bits(ens.V[valid]))
