"""CPU checks of the stress read-out's numpy restatement (tests/stress_ref.py), of the new
C-ABI symbols and of the scalar VTK writer.  No device needed.

The restatement is what tests/test_gpu_stress.py compares the kernels with bit for bit, so it
is anchored here on both sides: its pulls (bounce-back, NEE slots) reproduce the oracle's macros
of the next step bitwise, and its stress arithmetic gives the analytic 2 rho nu S on the
Chapman-Enskog populations of a uniform strain rate."""
import os
import subprocess

import numpy as np
import pytest

import stress_ref
from conftest import PKG


def _cases(oracle):
    from lbm_amd import cases
    geo = oracle.geo_ldc(16, 16, 16)
    yield "ldc16", geo, 3, (lambda: oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE))
    gp = oracle.geo_poiseuille(12, 16, 12)
    import lbm_amd
    yield "poiseuille", gp, 4, (lambda: oracle.Oracle(oracle.POISEUILLE, gp, 0.58))
    gd, bcs, _ = cases.duct_generic(24, 14, 12)
    yield "duct", gd, 4, (lambda: oracle.Oracle(oracle.GENERIC, gd, 0.6, bcs=bcs))
    raw = lbm_amd.read_geo_txt(os.path.join(cases.BIF_DIR, "geo.txt"))
    gb = lbm_amd.geo_mask(raw)
    _, inl, outl = lbm_amd.read_bc_txt(os.path.join(cases.BIF_DIR, "bc.txt"), gb, 1)
    yield "bifurcation", gb, 4, (lambda: oracle.Oracle(oracle.MASK, gb, 0.55, inlet_uy=inl, outlet_uy=outl))


@pytest.mark.parametrize("name", ["ldc16", "poiseuille", "duct", "bifurcation"])
def test_pull_reproduces_oracle_macros(oracle, lbm, name):
    """The restatement's pull of the oracle's populations after k - 1 steps gives, in k_moments'
    fp32 sums, the oracle's (rho, u) after k steps bit for bit on every fluid cell: bounce-back,
    NEE slots and direction numbering are the oracle's."""
    geo, fluid, make = next((g, f, m) for n, g, f, m in _cases(oracle) if n == name)
    o = make()
    fl = geo == fluid
    assert fl.any()
    for face in (fl[0], fl[-1], fl[:, 0], fl[:, -1], fl[:, :, 0], fl[:, :, -1]):
        assert not face.any()  # the restatement's shifts wrap: no fluid on a box face
    for k in range(1, 7):
        f_src = o.f()
        o.step(1)
        if k not in (1, 6):
            continue
        # only LDC bounces back at step 0; elsewhere the first step reads the wall slots raw
        got = stress_ref.macros32(stress_ref.pull(f_src, geo, raw_walls=(k == 1 and name != "ldc16")))
        for what, a, b in zip(("rho", "ux", "uy", "uz"), got, o.macros()):
            bad = np.count_nonzero(a[fl].view(np.uint32) != b[fl].view(np.uint32))
            assert bad == 0, f"{name} {what}: {bad} of {fl.sum()} fluid cells differ"


@pytest.mark.parametrize("rho,u", [(1.0, (0.0, 0.0, 0.0)), (1.03, (0.02, -0.01, 0.015))])
def test_uniform_shear_identity(rho, u):
    """On f_q = feq_q - 3 tau rho w_q (e_q e_q - delta/3):S rounded to fp32 the restatement returns
    sigma = 2 rho nu S, nu = (tau - 1/2)/3, and shear = sqrt(1/2 s':s') -- sign, factor and axis
    order, independent of any kernel.  atol = 2^-23 rho per component: each fp32-rounded population
    is off by at most 2^-24 f_q, enters a second moment with a coefficient of 0 or +-1, and
    sum f_q = rho, so P is within 2^-24 rho; r / 3 and m m / r (|u| << 1) add less than as much
    again, and |k| < 1.  Measured ~1e-9 (printed)."""
    tau = float(np.float32(0.6))
    S = 1e-3 * np.array([[0.7, 0.4, -0.3], [0.4, -0.2, 0.9], [-0.3, 0.9, -0.5]])
    f = stress_ref.uniform_shear_populations(rho, np.array(u), S, tau).astype(np.float32)
    f_src = np.broadcast_to(f[:, None, None, None], (19, 5, 5, 5)).copy()
    geo = np.full((5, 5, 5), 4, np.int8)
    r = stress_ref.stress_ref(f_src, geo, tau, 4)
    want = 2.0 * rho * ((tau - 0.5) / 3.0) * S
    atol = 2.0 ** -23 * rho
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        err = np.abs(r["stress"][k].astype(np.float64) - want[a, b]).max()
        print(f"uniform shear s{stress_ref.COMPONENTS[k]}: max error {err:.3e} (atol {atol:.3e})")
        assert err <= atol, (stress_ref.COMPONENTS[k], err)
    dev = want - np.trace(want) / 3.0 * np.eye(3)
    shear = np.sqrt(0.5 * np.sum(dev * dev))
    assert np.abs(r["shear"].astype(np.float64) - shear).max() <= atol
    assert r["n_wall"] == 0 and not r["shear_wall"].any() and r["n_fluid"] == 125


def test_stress_symbols_exported_and_bound(lbm):
    """lbm_get_stress / lbm_get_shear in liblbm.so, lbmh_write_vtk_scalar in liblbm_host.so, all
    three bound by the Python mirror with argument types."""
    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", lib)], capture_output=True,
                             text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"lbm_get_stress", "lbm_get_shear"} <= exported("liblbm.so")
    assert "lbmh_write_vtk_scalar" in exported("liblbm_host.so")
    assert {"lbm_get_stress", "lbm_get_shear"} <= set(lbm.LBM_SYMBOLS)
    assert "lbmh_write_vtk_scalar" in lbm.HOST_SYMBOLS
    assert len(lbm.lbm_lib().lbm_get_stress.argtypes) == 9
    assert len(lbm.lbm_lib().lbm_get_shear.argtypes) == 6
    assert len(lbm.host_lib().lbmh_write_vtk_scalar.argtypes) == 8
    assert callable(lbm.Lattice.stress) and callable(lbm.Lattice.shear)
    # NULL context: LBM_ERR_ARG without touching a device
    assert lbm.lbm_lib().lbm_get_stress(None, 0, 1, None, None, None, None, None, None) == -1
    assert lbm.lbm_lib().lbm_get_shear(None, 0, 1, 1, None, None) == -1


def test_write_vtk_scalar_round_trip(lbm, tmp_path):
    nx, ny, nz = 7, 5, 3
    rng = np.random.default_rng(7)
    data = (rng.standard_normal((nz, ny, nx)) * 10.0 ** rng.integers(-9, 3, (nz, ny, nx))).astype(np.float32)
    data[0, 0, :3] = 0.0
    scale, ch = np.float32(8010.97), 6.1111e-05
    path = str(tmp_path / "wss_0.vtk")
    lbm.write_vtk_scalar(path, "WSS", data, float(scale), ch)
    lines = open(path).read().split("\n")
    assert lines[0].startswith("# vtk DataFile") and lines[2] == "ASCII"
    assert lines[3] == "DATASET STRUCTURED_POINTS"
    assert lines[4] == f"DIMENSIONS {nx} {ny} {nz}"
    assert lines[5] == "SPACING " + " ".join(["%g" % np.float32(ch)] * 3)
    assert lines[7] == f"POINT_DATA {nx * ny * nz}"
    assert lines[8] == "SCALARS WSS float" and lines[9] == "LOOKUP_TABLE default"
    tokens = " ".join(lines[10:]).split()
    assert len(tokens) == nx * ny * nz
    want = ["%g" % float(v) for v in (data * scale).reshape(-1)]  # the fp32 product, x fastest
    assert tokens == want
    with pytest.raises(lbm.LbmError):
        lbm.write_vtk_scalar(str(tmp_path / "missing" / "x.vtk"), "WSS", data)
