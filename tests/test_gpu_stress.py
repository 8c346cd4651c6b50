"""lbm_get_stress / lbm_get_shear on the GPU: bit for bit against the numpy restatement
(tests/stress_ref.py) of the oracle's populations one step earlier, on every storage layout
(4- and 1-cell lanes, group lists, compact rows, both row axes, producer- and consumer-side
bounce-back), over plane ranges, slabs, the device-generated cavity, after a checkpoint, and
through bin/coronary --stress.  The read-outs leave the simulation state untouched."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import stress_ref
from conftest import PKG

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_RCCL, LBM_ERR_STATE = -1, -3, -4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    bad = np.count_nonzero(_bits(a) != _bits(b))
    assert bad == 0, f"{what}: {bad} of {np.asarray(a).size} values differ in their bits"


def _make(case, tau=None):
    """(lattice, geo, fluid code, tau, oracle factory) of a named case (tau: the box's, default 0.6)."""
    import orc
    from lbm_amd import cases
    kind, shape = case
    if kind == "box":
        tau = 0.6 if tau is None else tau
        geo, bcs, fields = cases.box_generic(*shape, 0)
        return cases.generic(geo, bcs, fields, tau=tau), geo, 4, tau, (lambda: orc.Oracle(orc.GENERIC, geo, tau, bcs=bcs))
    if kind == "ldc":
        lat, geo = cases.ldc(*shape)
        return lat, geo, 3, 0.55, (lambda: orc.Oracle(orc.LDC, geo, 0.55, ldc_order=orc.TWO_PHASE))
    if kind == "poiseuille":
        lat, geo = cases.poiseuille(*shape)
        return lat, geo, 4, 0.58, (lambda: orc.Oracle(orc.POISEUILLE, geo, 0.58))
    if kind == "duct":
        geo, bcs, fields = cases.duct_generic(*shape)
        return cases.generic(geo, bcs, fields, tau=0.6), geo, 4, 0.6, (lambda: orc.Oracle(orc.GENERIC, geo, 0.6, bcs=bcs))
    lat, geo, inl, outl = cases.bifurcation(1)
    return lat, geo, 4, 0.55, (lambda: orc.Oracle(orc.MASK, geo, 0.55, inlet_uy=inl, outlet_uy=outl))


@functools.lru_cache(maxsize=None)
def _reference(case, k, tau=None):
    """stress_ref of the oracle's populations after k - 1 steps: computed once per (case, k, tau) and
    shared by every layout (read-only)."""
    lat, geo, fluid, tau, make_oracle = _make(case, tau)
    lat.close()
    o = make_oracle()
    if k > 1:
        o.step(k - 1)
    ref = stress_ref.stress_ref(o.f(), geo, tau, fluid, raw_walls=(k == 1 and case[0] != "ldc"))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _check(lat, ref, what, zsl=slice(None)):
    s = lat.stress()
    for i, name in enumerate(stress_ref.COMPONENTS):
        _same(s[i], ref["stress"][i][zsl], f"{what} s{name}")
    sh, n = lat.shear(wall_only=False)
    _same(sh, ref["shear"][zsl], f"{what} shear")
    assert n == int(ref["fluid"][zsl].sum()), f"{what}: n_cells of the fluid"
    shw, nw = lat.shear(wall_only=True)
    _same(shw, ref["shear_wall"][zsl], f"{what} wall shear")
    assert nw == int(ref["wall"][zsl].sum()), f"{what}: n_cells of the wall"


CASES = [(("ldc", (16, 16, 16)), 1), (("ldc", (16, 16, 16)), 20), (("ldc", (37, 29, 23)), 17),
         (("poiseuille", (20, 16, 20)), 1), (("poiseuille", (20, 16, 20)), 30), (("poiseuille", (13, 11, 7)), 17),
         (("duct", (24, 14, 12)), 25), (("bifurcation", ()), 30), (("box", (21, 18, 15)), 11)]


@pytest.mark.parametrize("case,k", CASES, ids=[f"{c[0]}{'x'.join(map(str, c[1]))}-k{k}" for c, k in CASES])
def test_stress_bitwise(gpu, oracle, case, k, cells_per_lane, row_axis):
    """All six components, the shear everywhere and at the wall, n_cells and the exact zeros
    off-fluid equal the restatement's bits."""
    ref = _reference(case, k)
    assert ref["n_fluid"] > 0 and ref["n_wall"] > 0
    assert np.any(ref["stress"] != 0) and np.any(ref["shear_wall"] != 0)
    lat = _make(case)[0]
    lat.step(k, history=False)
    _check(lat, ref, f"{case} k={k}")
    lat.close()


@pytest.mark.parametrize("tau", [0.5, 1.0, 17.0])
def test_stress_tau(gpu, oracle, tau):
    """k = 1 - 0.5 / tau across tau on the six-face box (cfg 0) at step 11: tau 1.0 (k = 0.5) and
    17.0 bit for bit like test_stress_bitwise; at tau = 0.5 k = 0 and every component is a zero
    whose sign is that of the restatement's (-k) * N -- 7,841 negative zeros among the 6 x 2,618
    fluid values, 502 cells at the wall -- so the bits, signs included, still have to match."""
    case, k = ("box", (21, 18, 15)), 11
    ref = _reference(case, k, tau)
    assert (ref["n_fluid"], ref["n_wall"]) == (2618, 502)
    fl = ref["fluid"]
    if tau == 0.5:
        assert not ref["stress"].any() and not ref["shear"].any()
        assert 0 < np.count_nonzero(np.signbit(ref["stress"][:, fl])) < 6 * ref["n_fluid"]
    else:
        assert np.any(ref["stress"] != 0) and np.any(ref["shear_wall"] != 0)
    lat = _make(case, tau)[0]
    lat.step(k, history=False)
    _check(lat, ref, f"{case} k={k} tau={tau}")
    if tau == 0.5:
        assert not lat.stress().any() and not lat.shear(wall_only=False)[0].any() and not lat.shear()[0].any()
    lat.close()


def _layout(knob, gpu, which):
    """dense4: four cells per lane over whole chunks; compact1: one cell per lane in compact rows."""
    knob(gpu.TUNE_CELLS_PER_LANE, 4 if which == "dense4" else 1)
    knob(gpu.TUNE_GROUPS, 1 if which == "dense4" else 2)
    knob(gpu.TUNE_COMPACT, 1 if which == "dense4" else 2)


@pytest.mark.parametrize("which", ["dense4", "compact1"])
def test_plane_ranges(gpu, oracle, knob, which):
    """Ranges (0,1), (1,5), (5,nz) equal the whole-range read-out bitwise; ranges outside
    0 <= z0 < z1 <= nz are LBM_ERR_ARG."""
    _layout(knob, gpu, which)
    lat = _make(("bifurcation", ()))[0]
    assert lat.storage()["compact"] == (which == "compact1")
    lat.step(12, history=False)
    nz = lat.shape[0]
    s, (sh, n), (shw, nw) = lat.stress(), lat.shear(wall_only=False), lat.shear()
    assert n > nw > 0
    tot = totw = 0
    for z0, z1 in ((0, 1), (1, 5), (5, nz)):
        _same(lat.stress(z0, z1), s[:, z0:z1], f"stress planes {z0}:{z1}")
        a, m = lat.shear(z0, z1, wall_only=False)
        _same(a, sh[z0:z1], f"shear planes {z0}:{z1}")
        b, mw = lat.shear(z0, z1)
        _same(b, shw[z0:z1], f"wall shear planes {z0}:{z1}")
        assert m == np.count_nonzero(lat.geo()[z0:z1] == 4)
        tot, totw = tot + m, totw + mw
    assert (tot, totw) == (n, nw)
    L, buf = gpu.lbm_lib(), np.zeros((nz + 2,) + lat.shape[1:], np.float32)
    p = buf.ctypes.data_as(gpu.f32p)
    for z0, z1 in ((-1, 3), (0, nz + 1), (3, 3), (5, 2), (nz, nz + 1)):
        assert L.lbm_get_stress(lat.h, z0, z1, p, None, None, None, None, None) == LBM_ERR_ARG, (z0, z1)
        assert L.lbm_get_shear(lat.h, z0, z1, 1, p, None) == LBM_ERR_ARG, (z0, z1)
        with pytest.raises(gpu.LbmError, match="plane range"):
            lat.stress(z0, z1)
    assert not buf.any()
    lat.close()


def test_slabs_poiseuille(gpu, row_axis):
    """Three loopback slabs (ghost planes, halo exchange) equal the single-domain slices."""
    from lbm_amd import cases, initial_fields, Lattice, LBM_CASE_POISEUILLE, LBM_INIT_EXPANDED
    import lbm_amd
    nx, ny, nz = 24, 30, 33
    one, geo = cases.poiseuille(nx, ny, nz)
    prof = lbm_amd.poiseuille_profile(nx, nz)
    rho, ux, uy, uz = initial_fields(1, geo)
    xa = lbm_amd.x_align_for(geo, LBM_CASE_POISEUILLE)
    slabs = []
    for i in range(3):
        z0, z1 = cases.slab_bounds(nz, 3, i)
        lat = Lattice(LBM_CASE_POISEUILLE, (z1 - z0, ny, nx), 0.58, cases.slab_geo(geo, z0, z1), halo_planes=True,
                      inlet_uy=prof, outlet_uy=prof, z_offset=z0, nz_global=nz, x_align=xa)
        lat.init_equilibrium(LBM_INIT_EXPANDED, rho[z0:z1], ux[z0:z1], uy[z0:z1], uz[z0:z1])
        slabs.append((z0, z1, lat))
    one.step(45, history=False)
    lbm_amd.group_step([s[2] for s in slabs], 45, history=False)
    _slabs_equal(one, slabs)


def test_slabs_ldc_device(gpu):
    """The device-generated cavity in uneven slabs, a one-plane slab included."""
    from lbm_amd import cases
    import lbm_amd
    one = cases.ldc_device(20, 18, 7)
    slabs = [(z0, z1, cases.ldc_device(20, 18, z1 - z0, z_offset=z0, nz_global=7))
             for z0, z1 in ((0, 1), (1, 3), (3, 4), (4, 7))]
    one.step(25, history=False)
    lbm_amd.group_step([s[2] for s in slabs], 25, history=False)
    _slabs_equal(one, slabs)


def _slabs_equal(one, slabs):
    s, (sh, n), (shw, nw) = one.stress(), one.shear(wall_only=False), one.shear()
    assert np.any(s != 0) and nw > 0
    tot = totw = 0
    for z0, z1, lat in slabs:
        _same(lat.stress(), s[:, z0:z1], f"slab {z0}:{z1} stress")
        a, m = lat.shear(wall_only=False)
        _same(a, sh[z0:z1], f"slab {z0}:{z1} shear")
        b, mw = lat.shear()
        _same(b, shw[z0:z1], f"slab {z0}:{z1} wall shear")
        tot, totw = tot + m, totw + mw
        lat.close()
    assert (tot, totw) == (n, nw)
    one.close()


def test_device_generated_cavity_equals_host_geo(gpu):
    from lbm_amd import cases
    a, geo = cases.ldc(32, 32, 40)
    b = cases.ldc_device(32, 32, 40)
    a.step(30, history=False)
    b.step(30, history=False)
    _same(a.stress(), b.stress(), "stress")
    (sa, na), (sb, nb) = a.shear(), b.shear()
    _same(sa, sb, "wall shear")
    assert na == nb == int((stress_ref.wall_adjacent(geo) & (geo == 3)).sum())
    a.close()
    b.close()


@pytest.mark.parametrize("which", ["dense4", "compact1"])
def test_read_out_is_not_intrusive(gpu, oracle, knob, which):
    """Step 5, read stress and shear, step 5 more: populations and macros equal the oracle at 10
    and a twin that was never read; two consecutive reads are equal; macros() after stress() are
    still the oracle's."""
    from test_gpu_parity import assert_bitwise
    _layout(knob, gpu, which)
    case = ("bifurcation", ())
    lat, geo, fluid, tau, make_oracle = _make(case)
    twin = _make(case)[0]
    assert lat.storage()["compact"] == (which == "compact1")
    o = make_oracle()
    lat.step(5, history=False)
    twin.step(5, history=False)
    o.step(5)
    s1, (w1, n1) = lat.stress(), lat.shear()
    s2, (w2, n2) = lat.stress(), lat.shear()
    _same(s1, s2, "two reads: stress")
    _same(w1, w2, "two reads: wall shear")
    assert n1 == n2
    assert_bitwise(lat, o, geo, 2, "macros after stress()")
    _same(lat.stress(), s1, "stress after macros()")
    lat.step(5, history=False)
    twin.step(5, history=False)
    o.step(5)
    assert_bitwise(lat, o, geo, 2, "10 steps with a read-out in between")
    fl = geo == fluid
    _same(lat.f()[:, fl], twin.f()[:, fl], "populations against the unread twin")
    for a, b in zip(lat.macros(), twin.macros()):
        _same(a, b, "macros against the unread twin")
    _same(lat.stress(), twin.stress(), "stress against the unread twin")
    lat.close()
    twin.close()


def test_errors(gpu):
    from lbm_amd import cases
    import lbm_amd
    lat, _ = cases.ldc(16)
    L = gpu.lbm_lib()
    buf = np.zeros(lat.shape, np.float32)
    p = buf.ctypes.data_as(gpu.f32p)
    assert L.lbm_get_stress(lat.h, 0, 16, p, None, None, None, None, None) == LBM_ERR_STATE
    assert L.lbm_get_shear(lat.h, 0, 16, 1, p, None) == LBM_ERR_STATE
    with pytest.raises(gpu.LbmError, match="no step"):
        lat.stress()
    lat.step(1, history=False)
    assert np.any(lat.stress() != 0)
    lat.close()
    r = cases.ldc_device(24, 24, 24)
    r.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    r.step(3)
    r.sync()
    assert np.any(r.stress() != 0)
    r.debug_fail_next_wait()
    buf = np.zeros(r.shape, np.float32)
    p = buf.ctypes.data_as(gpu.f32p)
    assert L.lbm_get_stress(r.h, 0, 24, p, None, None, None, None, None) == LBM_ERR_RCCL
    assert L.lbm_get_shear(r.h, 0, 24, 1, p, None) == LBM_ERR_RCCL  # sticky
    with pytest.raises(gpu.LbmError, match="aborted"):
        r.shear()
    r.close()


def test_checkpoint(gpu, tmp_path):
    """A context that loaded a checkpoint taken at k = 12 reads the saver's stress without stepping."""
    a = _make(("poiseuille", (20, 16, 20)))[0]
    a.step(12, history=False)
    path = str(tmp_path / "k12.ckpt")
    a.checkpoint_save(path)
    b = _make(("poiseuille", (20, 16, 20)))[0]
    b.checkpoint_load(path)
    _same(b.stress(), a.stress(), "stress after checkpoint_load")
    (sa, na), (sb, nb) = a.shear(), b.shear()
    _same(sb, sa, "wall shear after checkpoint_load")
    assert na == nb > 0
    a.close()
    b.close()


def _run_coronary(tmp_path, out, extra):
    from lbm_amd import cases
    raw, ends = cases.coronary_small_vessel()
    nz, ny, nx = raw.shape
    if not (tmp_path / "geo.txt").exists():
        (tmp_path / "geo.txt").write_text(" ".join(map(str, raw.transpose(0, 2, 1).reshape(-1).tolist())))
    table = ";".join(",".join(map(str, e)) for e in ends)
    return subprocess.run([os.path.join(PKG, "bin", "coronary"), "--nx", str(nx), "--ny", str(ny), "--nz", str(nz),
                           "--ends", table, "--repeat", "10", "--time-save", "5", "--out", out] + extra,
                          cwd=tmp_path, capture_output=True, text=True, timeout=300, check=True)


def test_coronary_driver_stress(gpu, tmp_path):
    """bin/coronary --stress writes wss_<k>.vtk = lbm_get_shear(wall_only) * C_pre at every save
    step (to %g's six digits); without the flag no such file, and everything else the same bytes."""
    from lbm_amd import cases
    flagged = _run_coronary(tmp_path, "out_s", ["--stress"])
    plain = _run_coronary(tmp_path, "out_p", [])
    assert sorted(os.listdir(tmp_path / "out_p")) == ["CONVERGENCE.log"] + [f"coronary_{k}.vtk" for k in (0, 10, 5)]
    assert sorted(os.listdir(tmp_path / "out_s")) == sorted(os.listdir(tmp_path / "out_p") + [f"wss_{k}.vtk" for k in (0, 5, 10)])
    for k in (0, 5, 10):
        assert (tmp_path / "out_s" / f"coronary_{k}.vtk").read_bytes() == (tmp_path / "out_p" / f"coronary_{k}.vtk").read_bytes()

    def untimed(text):
        return re.sub(r"(collapse time: |TOTAL RUNNING TIME: )[0-9.e+-]+", r"\1T", text)
    assert untimed(flagged.stdout) == untimed(plain.stdout)
    logs = [(tmp_path / d / "CONVERGENCE.log").read_text().splitlines() for d in ("out_s", "out_p")]
    assert logs[0][:-1] == logs[1][:-1] and len(logs[0]) == 4
    raw, ends = cases.coronary_small_vessel()
    lat, geo = cases.coronary(raw, ends)
    nz, ny, nx = geo.shape
    cu, crho = np.float32(cases.CORONARY_C_U), np.float32(cases.CORONARY_C_RHO)
    c_pre = crho * cu * cu  # the driver's float product
    done = 0
    for k in (0, 5, 10):
        lat.step(k + 1 - done, history=False)
        done = k + 1
        want, n = lat.shear(wall_only=True)
        assert n > 0
        lines = (tmp_path / "out_s" / f"wss_{k}.vtk").read_text().split("\n")
        assert lines[4] == f"DIMENSIONS {nx} {ny} {nz}" and lines[8] == "SCALARS WSS float"
        got = np.array(" ".join(lines[10:]).split(), np.float64).reshape(geo.shape)
        np.testing.assert_allclose(got, (want * c_pre).astype(np.float64), rtol=1e-5, atol=0)
        assert np.count_nonzero(got) == np.count_nonzero(want)
    lat.close()
