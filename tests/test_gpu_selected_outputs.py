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
