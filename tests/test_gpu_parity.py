"""HIP path (liblbm.so through its C ABI) against the CPU oracle, on the GPU box.

Bar: bit-exact fp32 (rho, u) and populations on every fluid cell at identical step
counts -- stricter than the north star's 1e-6 relative L2, which is also reported.
The oracle restates the reference's two-pass algorithm (update kernel, then a boundary
pass that writes bounce-back / NEE values into boundary cells); liblbm evaluates the
boundaries on the consumer side inside one fused kernel, so equality here also proves
that re-formulation exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLUID = {0: 3, 1: 4, 2: 4}


def relL2(a, b):
    n = np.linalg.norm(b.astype(np.float64))
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / (n if n > 0 else 1.0))


def assert_bitwise(lat, o, geo, kind, what=""):
    m = geo == FLUID[kind]
    g = lat.macros()
    r = o.macros()
    for name, a, b in zip(("rho", "ux", "uy", "uz"), g, r):
        ga, ob = a[m], b[m]
        bad = np.count_nonzero(ga.view(np.uint32) != ob.view(np.uint32))
        assert bad == 0, f"{what} {name}: {bad} of {m.sum()} fluid cells differ (relL2 {relL2(ga, ob):.3e})"
    uf = np.stack(g[1:])[:, m]
    ur = np.stack(r[1:])[:, m]
    assert relL2(uf, ur) <= 1e-6 and relL2(g[0][m], r[0][m]) <= 1e-6
    fg, fr = lat.f(), o.f()
    bad = np.count_nonzero(fg[:, m].view(np.uint32) != fr[:, m].view(np.uint32))
    assert bad == 0, f"{what} f: {bad} fluid populations differ"


def assert_residuals(hg, ho):
    """Residual histories against an oracle switched to liblbm's summation (residual_fp64: the
    fp32 |u| terms, bit-identical here, summed in fp64).  Only the order of the fp64 additions
    differs, so S_k rounds to the same fp32 value and the residuals agree to the last bits; the
    tolerance admits one fp32 ulp of S_k (residual ~6e-8).  The reference's own fp32 thrust
    order is pinned separately, bit for bit, by the CUB-tree mode
    (test_gpu_configs.py::test_reference_order_residual_*)."""
    assert np.all(np.isfinite(hg))
    np.testing.assert_allclose(np.asarray(hg, np.float64), np.asarray(ho, np.float64), rtol=0, atol=1.2e-7)


def fp64_sum(o):
    """The oracle with liblbm's residual summation (see assert_residuals)."""
    o.residual_fp64(True)
    return o


@pytest.mark.parametrize("n,steps", [(16, [1, 1, 5, 40]), (32, [1, 3, 100]), (64, [2, 150])])
def test_ldc_bitwise(gpu, oracle, n, steps, cells_per_lane, row_axis):
    from lbm_amd import cases
    lat, geo = cases.ldc(n)
    o = fp64_sum(oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE))
    for s in steps:
        hg = lat.step(s)
        ho = o.step(s)
        assert_bitwise(lat, o, geo, 0, f"ldc{n} +{s}")
        assert_residuals(hg, ho)


@pytest.mark.parametrize("axis", ["x", "y"])
def test_fast_division_domain_retry(gpu, oracle, knob, axis):
    """Populations outside the fast quotient's proven domain (a tiny f, a huge f) make their
    waves take the exact division in the same launch: still bit-identical, and those chunk
    waves are counted.  Cells chosen next to the lid (NEE fix-up) and a wall."""
    from lbm_amd import cases
    knob(gpu.TUNE_CELLS_PER_LANE, 4)  # the fast division lives on the 4-cell path
    knob(gpu.TUNE_ROW_AXIS, 1 if axis == "x" else 2)
    n = 32
    lat, geo = cases.ldc(n)
    assert lat.numerics()["fast_div"]
    o = oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE)
    f = o.f()
    f[5, 10, n - 3, 9] = 1e-30   # z, y, x: NEE-adjacent row (y = ny-3 next to the lid at ny-2)
    f[7, 2, 12, 2] = 3e-25       # wall-adjacent corner region
    f[11, 16, 16, 16] = 1e-38    # interior
    lat.set_f(f)
    o.set_f(f)
    for s in (1, 1, 3):
        lat.step(s)
        o.step(s)
        assert_bitwise(lat, o, geo, 0, "retry")
    assert lat.numerics()["retried_chunks"] >= 3


def test_exact_division_switch(gpu, oracle, knob):
    """LBM_TUNE_EXACT_DIV = 1 keeps the compiler's division; results are the same bits."""
    from lbm_amd import cases
    knob(gpu.TUNE_EXACT_DIV, 1)
    lat, geo = cases.ldc(24)
    assert not lat.numerics()["fast_div"]
    o = oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE)
    lat.step(30)
    o.step(30)
    assert_bitwise(lat, o, geo, 0, "exact div")


def test_initial_state_bitwise(gpu, oracle):
    """lbm_init_equilibrium reproduces both reference initialize() forms bit for bit."""
    from lbm_amd import cases
    lat, geo = cases.ldc(16)
    o = oracle.Oracle(oracle.LDC, geo, 0.55)
    assert np.array_equal(lat.f().view(np.uint32), o.f().view(np.uint32))
    lat, geo = cases.poiseuille(20, 16, 20)
    o = oracle.Oracle(oracle.POISEUILLE, geo, 0.58)
    stored = geo != 0
    assert np.array_equal(lat.f()[:, stored].view(np.uint32), o.f()[:, stored].view(np.uint32))


@pytest.mark.parametrize("shape,steps", [((32, 32, 32), [1, 2, 60]), ((24, 40, 24), [1, 90]),
                                         ((64, 64, 64), [1, 120])])
def test_poiseuille_bitwise(gpu, oracle, shape, steps, cells_per_lane, row_axis):
    from lbm_amd import cases
    nx, ny, nz = shape
    lat, geo = cases.poiseuille(nx, ny, nz)
    o = fp64_sum(oracle.Oracle(oracle.POISEUILLE, geo, 0.58))
    for s in steps:
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 1, f"poiseuille{shape}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0


@pytest.mark.parametrize("block", [0, 1])
def test_bifurcation_bitwise(gpu, oracle, block, cells_per_lane, row_axis):
    from lbm_amd import cases
    lat, geo, inl, outl = cases.bifurcation(block)
    o = oracle.Oracle(oracle.MASK, geo, 0.55, inlet_uy=inl, outlet_uy=outl)
    for s in (1, 2, 200):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 2, f"bif block {block}")
    assert o.bad_reads() == 0


def test_bifurcation_full_run(gpu, oracle):
    """The reference's whole 4401-step run (bifurcation.cu:1246) of the meaningful variant."""
    from lbm_amd import cases
    lat, geo, inl, outl = cases.bifurcation(1)
    o = oracle.Oracle(oracle.MASK, geo, 0.55, inlet_uy=inl, outlet_uy=outl)
    lat.step(4401, history=False)
    o.step(4401)
    assert_bitwise(lat, o, geo, 2, "bif 4401")
    rho, ux, uy, uz = lat.macros()
    fl = geo == 4
    umax = float(np.sqrt(ux ** 2 + uy ** 2 + uz ** 2)[fl].max())
    assert abs(umax - 0.224) < 5e-4  # SURVEY.md finding 6 (emulated reference run)


def test_ldc_128_bitwise(gpu, oracle):
    from lbm_amd import cases
    lat, geo = cases.ldc(128)
    o = oracle.Oracle(oracle.LDC, geo, 0.55)
    lat.step(12, history=False)
    o.step(12)
    assert_bitwise(lat, o, geo, 0, "ldc128")


def test_device_generated_ldc_equals_host(gpu):
    """geo=NULL + lbm_init_ldc (the benchmark path) == host geo_pre + initialize()."""
    from lbm_amd import cases
    a, geo = cases.ldc(40, 36, 44)
    b = cases.ldc_device(40, 36, 44)
    a.step(33, history=False)
    b.step(33, history=False)
    for x, y in zip(a.macros(), b.macros()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a.counts() == b.counts()


def test_convergence_loop(gpu, oracle):
    """Device-side stopping rule of ldc.cu:653-685 (k <= max_it && tol_count <= stag_max)."""
    from lbm_amd import cases
    lat, geo = cases.ldc(24)
    lat.set_convergence(True, max_it=10000, stag_max=50, tol=1e-6)
    o = oracle.Oracle(oracle.LDC, geo, 0.55)
    k_ref, _ = o.run_converge()
    done = 0
    while True:
        lat.step(500)
        st = lat.state()
        if st["stopped"]:
            break
        assert st["k"] < 20000
    k = st["k"]
    # the stop step depends on fp32 summation noise of |u| (thrust order in the reference)
    assert abs(k - k_ref) <= max(50, 0.05 * k_ref), (k, k_ref)
    # fields agree exactly once both stepped to the same k
    o2 = oracle.Oracle(oracle.LDC, geo, 0.55)
    o2.step(k)
    assert_bitwise(lat, o2, geo, 0, f"ldc24 converged at {k}")
    # further steps are no-ops
    lat.step(7)
    assert lat.state()["k"] == k


@pytest.mark.parametrize("nslabs", [2, 3])
def test_loopback_slabs_bitwise(gpu, nslabs, cells_per_lane, row_axis):
    """z-slab decomposition with halo exchange (5 populations per face) == one domain."""
    from lbm_amd import cases, initial_fields, Lattice, LBM_CASE_POISEUILLE, LBM_INIT_EXPANDED
    import lbm_amd
    nx, ny, nz = 24, 30, 33
    one, geo = cases.poiseuille(nx, ny, nz)
    prof = lbm_amd.poiseuille_profile(nx, nz)
    rho, ux, uy, uz = initial_fields(1, geo)
    xa = lbm_amd.x_align_for(geo, LBM_CASE_POISEUILLE)
    slabs = []
    for i in range(nslabs):
        z0, z1 = cases.slab_bounds(nz, nslabs, i)
        lat = Lattice(LBM_CASE_POISEUILLE, (z1 - z0, ny, nx), 0.58, cases.slab_geo(geo, z0, z1), halo_planes=True,
                      inlet_uy=prof, outlet_uy=prof, z_offset=z0, nz_global=nz, x_align=xa)
        lat.init_equilibrium(LBM_INIT_EXPANDED, rho[z0:z1], ux[z0:z1], uy[z0:z1], uz[z0:z1])
        slabs.append((z0, z1, lat))
    h1 = one.step(45)
    hs = lbm_amd.group_step([s[2] for s in slabs], 45)
    np.testing.assert_allclose(hs, h1, rtol=0, atol=1e-6)
    ref = one.macros()
    for z0, z1, lat in slabs:
        for a, b in zip(lat.macros(), ref):
            assert np.array_equal(a.view(np.uint32), b[z0:z1].view(np.uint32))


def test_loopback_ldc_device_slabs(gpu):
    from lbm_amd import cases
    import lbm_amd
    one = cases.ldc_device(32, 32, 40)
    slabs = [(z0, z1, cases.ldc_device(32, 32, z1 - z0, z_offset=z0, nz_global=40))
             for z0, z1 in (cases.slab_bounds(40, 4, i) for i in range(4))]
    one.step(30, history=False)
    lbm_amd.group_step([s[2] for s in slabs], 30, history=False)
    ref = one.macros()
    for z0, z1, lat in slabs:
        for a, b in zip(lat.macros(), ref):
            assert np.array_equal(a.view(np.uint32), b[z0:z1].view(np.uint32))


def test_large_box_properties(gpu):
    """512^3 (the north-star lattice, 20.4 GB of populations): runs, stays finite, is
    deterministic, and mass changes only through the lid."""
    from lbm_amd import cases
    hs = []
    for _ in range(2):
        lat = cases.ldc_device(512, 512, 512)
        assert lat.counts()["n_fluid"] == 508 ** 3
        hs.append(lat.step(6))
        st = lat.state()
        rho, ux, uy, uz = lat.macros()
        fl = rho != 0
        assert np.isfinite(st["velsum"]) and np.all(np.isfinite(rho[fl]))
        assert abs(float(rho[fl].mean()) - 1.0) < 1e-4
        lat.close()
        del lat, rho, ux, uy, uz
    assert np.array_equal(hs[0].view(np.uint32), hs[1].view(np.uint32))


@pytest.mark.parametrize("name", ["ldc16_two_phase", "poiseuille_20x24x20", "bif_inlet_block1"])
def test_matches_committed_golden(gpu, name):
    """liblbm against the committed golden vectors (tests/golden/make_golden.py), independent
    of the oracle build on the box."""
    import hashlib
    import json
    import os
    from conftest import GOLDEN
    import lbm_amd
    from lbm_amd import cases
    meta = json.load(open(os.path.join(GOLDEN, "golden.json")))[name]
    if name.startswith("ldc"):
        lat, geo = cases.ldc(16)
    elif name.startswith("poiseuille"):
        lat, geo = cases.poiseuille(20, 24, 20)
    else:
        lat, geo, _, _ = cases.bifurcation(1)
    lat.step(meta["steps"], history=False)
    rho, ux, uy, uz = lat.macros()
    fl = geo == FLUID[meta["kind"]]
    h = hashlib.sha256()
    for a in (rho[fl], ux[fl], uy[fl], uz[fl]):
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == meta["sha256_macros_fluid"]
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(lat.f()[:, fl]).tobytes())
    assert h.hexdigest() == meta["sha256_f_fluid"]
    lbm_amd  # noqa: B018


def test_fast_division_retry_large(gpu, oracle):
    """The same injected out-of-domain populations on LDC 256^3, where the per-block partials
    exceed the one-block reduction (the sliced reduction finishes the last step)."""
    from lbm_amd import cases
    n = 256
    lat, geo = cases.ldc(n)
    o = oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE)
    f = o.f()
    # each pulled by a chunk-wave fluid cell (y = n - 3 would be NEE-adjacent, under the lid:
    # the NEE blocks update it and the chunk wave's lane mask leaves it out)
    f[5, 100, n - 4, 17] = 1e-30
    f[7, 2, 140, 2] = 3e-25
    f[11, 200, 60, 201] = 7e-39
    lat.set_f(f)
    o.set_f(f)
    del f
    for s in (1, 2):
        lat.step(s, history=False)
        o.step(s)
    assert_bitwise(lat, o, geo, 0, "retry 256")
    assert lat.numerics()["retried_chunks"] >= 3


@pytest.mark.parametrize("shape", [(24, 14, 12), (40, 22, 18)])
def test_generic_boundaries_bitwise(gpu, oracle, shape, cells_per_lane, row_axis):
    """LBM_CASE_GENERIC: inlet (+x, velocity + rho, per-cell table), outlet (-x, velocity),
    side outlet (-z) and a pressure patch (+y) -- coronary.cu:716-944's scheme on every kind
    of face -- bit for bit against the oracle's generic restatement."""
    from lbm_amd import cases
    nx, ny, nz = shape
    geo, bcs, fields = cases.duct_generic(nx, ny, nz)
    lat = cases.generic(geo, bcs, fields, tau=0.6)
    o = fp64_sum(oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs))
    for s in (1, 1, 40):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 2, f"generic {shape} +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0


def test_coronary_codes_bitwise(gpu, oracle):
    """coronary.cu's own code table (cases.coronary_bc_codes: 2 inlet +x with rho 1, 3 outlet
    -x, 5/6/7 outlets -z) on a synthetic duct with three top-wall outlet patches."""
    from lbm_amd import cases
    nx, ny, nz = 30, 16, 14
    geo, _, (rho, ux, uy, uz) = cases.duct_generic(nx, ny, nz)
    geo[geo == 6] = 1
    geo[geo == 5] = 1
    for k, x0 in ((5, 5), (6, 12), (7, 20)):
        geo[nz - 2, 6:9, x0:x0 + 3] = k
    bcs = cases.coronary_bc_codes()
    ux = np.where(geo == 2, np.float32(bcs[0]["u"][0]), np.where(geo == 3, np.float32(bcs[1]["u"][0]), 0))
    uz = np.where((geo >= 5) & (geo <= 7), np.float32(bcs[2]["u"][2]), 0)
    fields = (rho, ux.astype(np.float32), uy, uz.astype(np.float32))
    lat = cases.generic(geo, bcs, fields, tau=0.6)
    o = fp64_sum(oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs))
    for s in (1, 60):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 2, f"coronary codes +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0


@pytest.mark.parametrize("shape", [(37, 29, 23), (13, 11, 7), (66, 9, 31)])
def test_ragged_shapes_bitwise(gpu, oracle, shape, cells_per_lane, row_axis):
    """Extents that are not multiples of 4 (row padding, row shift, chunks straddling rows
    and planes) and very flat boxes."""
    from lbm_amd import cases
    nx, ny, nz = shape
    lat, geo = cases.ldc(nx, ny, nz)
    o = oracle.Oracle(oracle.LDC, geo, 0.55)
    lat.step(17, history=False)
    o.step(17)
    assert_bitwise(lat, o, geo, 0, f"ldc {shape}")
    lat, geo = cases.poiseuille(nx, ny, nz)
    o = oracle.Oracle(oracle.POISEUILLE, geo, 0.58)
    lat.step(17, history=False)
    o.step(17)
    assert_bitwise(lat, o, geo, 1, f"poiseuille {shape}")


def test_thin_slabs_loopback(gpu, row_axis):
    """Slabs of one and two planes (edge ranges overlapping / covering the whole slab)."""
    from lbm_amd import cases
    import lbm_amd
    nz = 7
    one = cases.ldc_device(20, 18, nz)
    bounds = [(0, 1), (1, 3), (3, 4), (4, 7)]
    slabs = [(z0, z1, cases.ldc_device(20, 18, z1 - z0, z_offset=z0, nz_global=nz)) for z0, z1 in bounds]
    h1 = one.step(25)
    hs = lbm_amd.group_step([s[2] for s in slabs], 25)
    np.testing.assert_allclose(hs, h1, rtol=0, atol=1e-6)
    ref = one.macros()
    for z0, z1, lat in slabs:
        for a, b in zip(lat.macros(), ref):
            assert np.array_equal(a.view(np.uint32), b[z0:z1].view(np.uint32))


def test_rccl_single_rank_step_path(gpu, cells_per_lane, row_axis):
    """lbm_attach_rccl with one rank: the multi-GPU step (edge planes then interior on two
    streams, halo pack/unpack, residual all-reduce + device finisher) with no peers -- must
    match the single-domain step bit for bit, residuals included."""
    from lbm_amd import cases
    import lbm_amd
    a = cases.ldc_device(40, 36, 44)
    b = cases.ldc_device(40, 36, 44)
    b.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    ha = a.step(35)
    hb = b.step(35)
    assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32))
    for x, y in zip(a.macros(), b.macros()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # convergence control through the RCCL finisher
    a.set_convergence(True, max_it=60, stag_max=50, tol=1e-6)
    b.set_convergence(True, max_it=60, stag_max=50, tol=1e-6)
    a.step(100)
    b.step(100)
    assert a.state()["k"] == b.state()["k"] == 61
    b.close()


def test_row_axis_choice(gpu, oracle):
    """lbm_desc.row_axis = 0 picks rows along y for a pipe along y (whole fluid rows: fewer
    active chunks) and x for the cavity; an explicit row_axis in the descriptor is honoured
    and bit-identical to the oracle."""
    from lbm_amd import cases, Lattice, LBM_CASE_LDC, LBM_INIT_LDC_WI, initial_fields
    lat, geo = cases.poiseuille(32, 256, 32)
    lay = lat.layout()
    assert lay["row_axis"] == 2 and lay["pitch"] == 256, lay
    geo_x = Lattice(lat.case_kind, geo.shape, 0.58, geo, row_axis=1).layout()
    assert lay["active_chunks"] < 0.8 * geo_x["active_chunks"], (lay, geo_x)
    lat, _ = cases.ldc(24)
    assert lat.layout()["row_axis"] == 1
    assert cases.ldc_device(24, 24, 24).layout()["row_axis"] == 1
    geo = __import__("lbm_amd").geo_ldc(22, 30, 26)
    lat = Lattice(LBM_CASE_LDC, geo.shape, 0.55, geo, row_axis=2)
    assert lat.layout()["row_axis"] == 2 and lat.layout()["pitch"] == 32
    lat.init_equilibrium(LBM_INIT_LDC_WI, *initial_fields(0, geo))
    o = oracle.Oracle(oracle.LDC, geo, 0.55)
    lat.step(21, history=False)
    o.step(21)
    assert_bitwise(lat, o, geo, 0, "ldc row_axis 2")


def test_poiseuille_c3_full_size_bitwise(gpu, oracle):
    """BASELINE config C3 at its full size (128 x 512 x 128, pipe along y, 6.7 M stored cells),
    bit for bit against the oracle after 1 and 3 steps (populations included)."""
    from lbm_amd import cases
    lat, geo = cases.poiseuille(128, 512, 128)
    o = fp64_sum(oracle.Oracle(oracle.POISEUILLE, geo, 0.58))
    for s in (1, 2):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 1, f"C3 +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0


@pytest.mark.parametrize("nee_fix", [3, 1, 2], ids=["nee_fix", "nee_blocks", "nee_records"])
@pytest.mark.parametrize("shape", [(24, 40, 24), (33, 70, 29), (20, 512, 18), (17, 300, 21)])
def test_poiseuille_nee_paths_bitwise(gpu, oracle, knob, nee_fix, shape):
    """The pipe along y with four cells per lane: its chunk waves collide the NEE-adjacent cells
    (nee_chunks), and the NEE values come from NEE blocks that re-pull and re-collide those cells
    (LBM_TUNE_NEE_FIX 1, the default), from k_nee_fix after the step launch (3), or from NEE records
    (2, where the chunk list carries no lane masks and every chunk holds at most 8 NEE-adjacent
    cells: the rows of 512 cells, two whole chunks each; the 40-, 70- and 300-cell rows fall back
    to k_nee_fix, see test_gpu_tau.py).  All bit for bit against the oracle, populations
    included (the read-outs put the records' values into the NEE cells' slots), through the
    convergence-free loop and a convergence-controlled one (no-op steps after the stop write no
    record and launch no k_nee_fix)."""
    from lbm_amd import cases
    import lbm_amd
    knob(lbm_amd.TUNE_CELLS_PER_LANE, 4)
    knob(lbm_amd.TUNE_NEE_FIX, nee_fix)
    nx, ny, nz = shape
    lat, geo = cases.poiseuille(nx, ny, nz)
    assert lat.layout()["row_axis"] == 2
    o = fp64_sum(oracle.Oracle(oracle.POISEUILLE, geo, 0.58))
    for s in (1, 2, 37):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 1, f"pipe {shape} +{s}")
        assert_residuals(hg, ho)
    lat.set_convergence(True, max_it=45, stag_max=50, tol=1e-6)
    lat.step(20)
    assert lat.state()["k"] == 46 and lat.state()["stopped"] == 1
    o.step(6)
    assert_bitwise(lat, o, geo, 1, f"pipe {shape} stopped at 46")


@pytest.mark.parametrize("shape,most", [((32, 32, 32), 8), ((37, 30, 23), 8), ((13, 47, 11), 6)])
def test_nee_records_full_chunks_bitwise(gpu, oracle, knob, shape, most):
    """NEE records (LBM_TUNE_NEE_FIX 2) on chunks holding up to eight records: the cavity with rows
    along y puts one lid-adjacent cell at the end of every row, so a 256-cell chunk of 32-cell rows
    holds eight.  Their static records are 8 x 9 = 72 float4, more than one 64-lane wave-load; in
    round 5 a single wave-load left the ninth float4 onward unloaded (LDC 32^3, 840 of 21,952 fluid
    cells wrong at step 3).  Bit for bit against the oracle, with the ragged
    shapes' padded rows (pitch 32 for 30 cells; 48 for 47: five or six rows per chunk).  Records
    need the chunk waves to collide the lid-adjacent cells (nee_chunks), so the row lengths put
    that cell in a 4-cell group with other fluid cells (ny - 5 not a multiple of 4)."""
    from lbm_amd import cases
    import lbm_amd
    knob(lbm_amd.TUNE_CELLS_PER_LANE, 4)
    knob(lbm_amd.TUNE_ROW_AXIS, 2)
    knob(lbm_amd.TUNE_NEE_FIX, 2)
    nx, ny, nz = shape
    lat, geo = cases.ldc(nx, ny, nz)
    assert lat.layout()["row_axis"] == 2
    assert lat.nee_path() == {"path": "records", "max_records": most}, lat.nee_path()
    o = fp64_sum(oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE))
    for s in (1, 2, 3, 40):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 0, f"ldc {shape} records +{s}")
        assert_residuals(hg, ho)


def test_north_star_512_bitwise(gpu, oracle):
    """The north-star lattice itself (LDC 512^3, the bench's N = 1 workload, generated on the
    device as bench.py does) against the oracle on the host: (rho, u) bit for bit on all
    131 M fluid cells after 3 steps.  The residual: liblbm's fp64 |u| sum equals an fp64 sum of
    the same (bit-identical) per-cell |u| to 1e-12, and the residual history equals the oracle's
    in the same summation to the last bits (assert_residuals).  The reference's fp32 thrust
    order would move it by ~2e-3 over 131 M terms (oracle/PINNING.md section 3)."""
    import lbm_amd
    from lbm_amd import cases
    n = 512
    lat = cases.ldc_device(n, n, n)
    hg = lat.step(3)
    velsum = lat.state()["velsum"]
    g = lat.macros()
    lat.close()
    del lat
    geo = lbm_amd.geo_ldc(n, n, n)
    o = fp64_sum(oracle.Oracle(oracle.LDC, geo, 0.55, ldc_order=oracle.TWO_PHASE))
    ho = o.step(3)
    r = o.macros()
    del o
    m = geo == 3
    del geo
    for name, a, b in zip(("rho", "ux", "uy", "uz"), g, r):
        bad = np.count_nonzero(a[m].view(np.uint32) != b[m].view(np.uint32))
        assert bad == 0, f"512^3 {name}: {bad} fluid cells differ"
    del r
    ux, uy, uz = (a[m] for a in g[1:])
    s64 = float(np.sqrt(ux * ux + uy * uy + uz * uz).astype(np.float64).sum())
    assert abs(velsum - s64) <= 1e-12 * s64, (velsum, s64)
    assert_residuals(hg, ho)


def test_rccl_abort_is_sticky(gpu, knob):
    """A wait that sees a failed peer aborts the communicator (here injected with
    lbm_debug_fail_next_wait on a one-rank RCCL slab; a second context is not affected).  From then on the context refuses to
    step, wait, read out or checkpoint with LBM_ERR_RCCL -- it does not fall back to stepping
    the slab as a single domain with stale ghost planes."""
    from lbm_amd import cases, LbmError
    import lbm_amd
    lat = cases.ldc_device(24, 24, 24)
    lat.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    lat.step(3)
    lat.step(2, history=False)
    lat.sync()  # streams drained: the abort below finds no work in flight
    other = cases.ldc_device(16, 16, 16)
    other.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    lat.debug_fail_next_wait()
    other.step(2)
    other.sync()  # the hook is per context: this one waits normally
    with pytest.raises(LbmError, match="RCCL peer failure"):
        lat.sync()
    other.step(1)
    other.close()
    for call in (lambda: lat.step(1), lat.sync, lat.macros, lat.state, lat.comm_info, lat.f,
                 lambda: lat.checkpoint_save("/tmp/never_written.bin")):
        with pytest.raises(LbmError, match="aborted"):
            call()
    lat.close()
