"""LBM_CASE_GENERIC on all six faces and three kinds (cases.box_generic), bit for bit against the
CPU oracle: every stream-collide path, the NEE paths of the 4-cell kernel, z-slabs whose cuts fall
between a z-face NEE plane and its fluid plane, and the RCCL step path with one rank.

tests/test_generic_box.py (CPU) shows that these comparisons depend on every face's table raster."""
import numpy as np
import pytest

from test_gpu_parity import assert_bitwise, assert_residuals, fp64_sum

pytestmark = pytest.mark.gpu

SHAPES = [(21, 18, 15), (14, 23, 19), (13, 11, 12)]  # (nx, ny, nz)
Q_E = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0),
       (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    bad = np.count_nonzero(_bits(a) != _bits(b))
    assert bad == 0, f"{what}: {bad} of {np.asarray(a).size} values differ in their bits"


def nee_adjacent_cells(geo, bcs):
    """Fluid cells c with, for some direction q, an NEE cell at c - e_q whose face takes q
    (e_q along the face's axis points into the fluid)."""
    fl = geo == 4
    adj = np.zeros(geo.shape, bool)
    for b in bcs:
        axis, sign = b["face"] >> 1, 1 if b["face"] % 2 == 0 else -1
        cells = geo == b["code"]
        for ex, ey, ez in Q_E[1:]:
            if (ex, ey, ez)[axis] == sign:
                adj |= np.roll(cells, (ez, ey, ex), axis=(0, 1, 2))  # cells(c - e_q)
    return adj & fl


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_box_every_face_and_kind_bitwise(gpu, oracle, shape, cfg, cells_per_lane, row_axis):
    """Each of the 18 (face, kind) pairs, with per-cell tables on x, y and z faces, through every
    stream-collide path and both row axes."""
    from lbm_amd import cases
    geo, bcs, fields = cases.box_generic(*shape, cfg)
    lat = cases.generic(geo, bcs, fields, tau=0.6)
    o = fp64_sum(oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs))
    assert lat.counts()["n_boundary"] == int(nee_adjacent_cells(geo, bcs).sum())
    assert lat.counts()["n_fluid"] == int((geo == 4).sum())
    for s in (1, 1, 2, 36):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 2, f"box {shape} cfg {cfg} +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0
    lat.close()


# what lbm.h documents for LBM_TUNE_NEE_FIX: 1 NEE blocks; 3 k_nee_fix where the chunk waves collide
# the NEE-adjacent cells, NEE blocks elsewhere; 2 records on chunk lists with at most 8 such cells
# per chunk, "otherwise as 3"
NEE_PATHS = {1: ("blocks",), 3: ("fix", "blocks"), 2: ("records", "fix", "blocks")}


@pytest.mark.parametrize("nee_fix", [1, 3, 2], ids=["nee_blocks", "nee_fix", "nee_records"])
@pytest.mark.parametrize("shape,cfg", [((21, 18, 15), 0), ((14, 23, 19), 1)], ids=["21x18x15-cfg0", "14x23x19-cfg1"])
def test_box_nee_paths_bitwise(gpu, oracle, knob, shape, cfg, nee_fix, row_axis):
    """The three ways the 4-cell kernel produces NEE values, on cells with NEE neighbours on up to
    two faces of different kinds; then the convergence-controlled stop (no-op steps write nothing)."""
    from lbm_amd import cases
    import lbm_amd
    knob(lbm_amd.TUNE_CELLS_PER_LANE, 4)
    knob(lbm_amd.TUNE_NEE_FIX, nee_fix)
    geo, bcs, fields = cases.box_generic(*shape, cfg)
    lat = cases.generic(geo, bcs, fields, tau=0.6)
    path = lat.nee_path()
    print(f"nee_path {shape} cfg {cfg} rows {row_axis} LBM_TUNE_NEE_FIX {nee_fix}: {path}")
    assert path["path"] in NEE_PATHS[nee_fix], path
    assert (1 <= path["max_records"] <= 8) if path["path"] == "records" else path["max_records"] == 0, path
    assert lat.launch_shape()["cells_per_lane"] == 4
    o = fp64_sum(oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs))
    for s in (1, 2, 3, 30):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 2, f"box {shape} cfg {cfg} {path['path']} +{s}")
        assert_residuals(hg, ho)
    lat.set_convergence(True, max_it=36, stag_max=50, tol=1e-6)
    lat.step(20)
    assert lat.state()["k"] == 37 and lat.state()["stopped"] == 1
    o.step(1)
    assert_bitwise(lat, o, geo, 2, f"box {shape} cfg {cfg} stopped at 37")
    assert o.bad_reads() == 0
    lat.close()


NZ = 15
BOUNDS = {
    # cuts exactly between each z-face NEE plane and its fluid plane (1|2, 12|13) and at the end
    # of the NX patch; the end slabs hold no fluid
    "nee_plane_cuts": [(0, 2), (2, 8), (8, 13), (13, 15)],
    # one- and two-plane slabs, one cut through the x and y patches
    "thin": [(0, 1), (1, 3), (3, 7), (7, 14), (14, 15)],
    "even2": None,
    "even3": None,
}


def _bounds(name):
    from lbm_amd import cases
    if BOUNDS[name] is not None:
        return BOUNDS[name]
    n = int(name[-1])
    return [cases.slab_bounds(NZ, n, i) for i in range(n)]


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("bounds", list(BOUNDS))
def test_box_slabs_bitwise(gpu, oracle, bounds, cfg, row_axis):
    """The box as loopback z-slabs (ghost planes, 5 populations per face exchanged each step) equals
    the single domain, which equals the oracle.  A z-face NEE cell in a ghost plane keeps the values
    its local fluid neighbour stored (k_unpack skips NEE ghost cells); the x- and y-face tables are
    read at the global z."""
    from lbm_amd import cases, Lattice, LBM_CASE_GENERIC, LBM_INIT_EXPANDED
    import lbm_amd
    nx, ny, nz = 21, 18, NZ
    geo, bcs, fields = cases.box_generic(nx, ny, nz, cfg)
    fl = geo == 4
    one = cases.generic(geo, bcs, fields, tau=0.6)
    o = fp64_sum(oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs))
    xa = lbm_amd.x_align_for(geo, LBM_CASE_GENERIC)
    slabs = []
    for z0, z1 in _bounds(bounds):
        lat = Lattice(LBM_CASE_GENERIC, (z1 - z0, ny, nx), 0.6, cases.slab_geo(geo, z0, z1), halo_planes=True,
                      z_offset=z0, nz_global=nz, x_align=xa, bc_codes=bcs)
        lat.init_equilibrium(LBM_INIT_EXPANDED, *[a[z0:z1] for a in fields])
        slabs.append((z0, z1, lat))
    assert sum(s[2].counts()["n_fluid"] for s in slabs) == int(fl.sum())
    assert sum(s[2].counts()["n_boundary"] for s in slabs) == one.counts()["n_boundary"]
    for steps in (1, 2, 30):
        h1, ho = one.step(steps), o.step(steps)
        hs = lbm_amd.group_step([s[2] for s in slabs], steps)
        assert_bitwise(one, o, geo, 2, f"box cfg {cfg} single domain +{steps}")
        assert_residuals(h1, ho)
        np.testing.assert_allclose(hs, h1, rtol=0, atol=1e-6)
        ref_m, ref_f, ref_s, (ref_w, ref_nw), ref_d = one.macros(), one.f(), one.stress(), one.shear(), one.digest()
        assert np.any(ref_s[:, fl] != 0) and ref_nw > 0
        nw = 0
        for z0, z1, lat in slabs:
            what = f"box cfg {cfg} slab {z0}:{z1} +{steps}"
            m = fl[z0:z1]
            for name, a, b in zip(("rho", "ux", "uy", "uz"), lat.macros(), ref_m):
                _same(a[m], b[z0:z1][m], f"{what} {name}")
            _same(lat.f()[:, m], ref_f[:, z0:z1][:, m], f"{what} f")
            _same(lat.stress()[:, m], ref_s[:, z0:z1][:, m], f"{what} stress")
            w, n = lat.shear(wall_only=True)
            _same(w[m], ref_w[z0:z1][m], f"{what} wall shear")
            nw += n
            assert np.array_equal(lat.digest(), ref_d[z0:z1]), f"{what} digest"
        assert nw == ref_nw
    assert o.bad_reads() == 0
    for _, _, lat in slabs:
        lat.close()
    one.close()


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_box_rccl_single_rank(gpu, knob, cfg):
    """lbm_attach_rccl with one rank on the box: edge and interior launches on two streams, pack
    and unpack with no peer -- bit-identical to the unattached lattice, residual history included."""
    from lbm_amd import cases
    import lbm_amd
    knob(lbm_amd.TUNE_COMPACT, 1)  # a lattice in compact rows cannot attach (lbm.h)
    geo, bcs, fields = cases.box_generic(21, 18, 15, cfg)
    a = cases.generic(geo, bcs, fields, tau=0.6)
    b = cases.generic(geo, bcs, fields, tau=0.6)
    b.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    ha, hb = a.step(25), b.step(25)
    _same(ha, hb, "residual history")
    for name, x, y in zip(("rho", "ux", "uy", "uz"), a.macros(), b.macros()):
        _same(x, y, name)
    fl = geo == 4
    _same(a.f()[:, fl], b.f()[:, fl], "f")
    assert np.any(a.macros()[1][fl] != 0)
    b.close()
    a.close()
