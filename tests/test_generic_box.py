"""cases.box_generic on the CPU oracle: the six-face LBM_CASE_GENERIC box that
tests/test_gpu_generic.py compares the kernels on.  No device needed.

These checks show that the GPU comparisons are able to fail: the three configurations hold each
(face, kind) pair once, every code is present at every shape used, the run stays finite, and the
oracle's result depends on every face's table raster -- a transposed or flipped table changes
(rho, u) bits within three steps -- while a pressure code's table changes nothing."""
import functools

import numpy as np
import pytest

SHAPES = [(21, 18, 15), (14, 23, 19), (13, 11, 12)]  # (nx, ny, nz), as in test_gpu_generic.py
FACE_NAMES = ("PX", "NX", "PY", "NY", "PZ", "NZ")
Q_EX = (0, 1, -1, 0, 0, 0, 0, 1, 1, -1, -1, 1, 1, -1, -1, 0, 0, 0, 0)
Q_EY = (0, 0, 0, 1, -1, 0, 0, 1, -1, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1)
Q_EZ = (0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1, 1, 1, -1, -1)


def _bits(arrs, m):
    return np.stack([np.ascontiguousarray(a[m]).view(np.uint32) for a in arrs])


def _macro_bits(oracle, geo, bcs, steps):
    o = oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs)
    o.step(steps)
    return _bits(o.macros(), geo == 4)


def test_configurations_cover_every_face_and_kind(lbm):
    from lbm_amd import cases
    seen = []
    for cfg in range(3):
        _, bcs, _ = cases.box_generic(*SHAPES[0], cfg)
        assert [b["face"] for b in bcs] == list(range(6))
        assert [b["code"] for b in bcs] == list(cases.BOX_CODES)
        seen += [(b["face"], b["kind"]) for b in bcs]
    assert sorted(seen) == [(f, k) for f in range(6) for k in range(3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_geometry(lbm, shape):
    """Every code present; each patch lies in its wall with the fluid on the face's side; the table
    rasters have the face's extents and differ from their transposes and flips on the patch."""
    from lbm_amd import cases
    nx, ny, nz = shape
    geo, bcs, fields = cases.box_generic(nx, ny, nz, 0)
    assert geo.shape == (nz, ny, nx) and geo.dtype == np.int8
    assert set(np.unique(geo)) == {0, 1, 4} | set(cases.BOX_CODES)
    assert np.count_nonzero(geo == 4) == (nx - 4) * (ny - 4) * (nz - 4)
    for b in bcs:
        f = b["face"]
        axis, sign = f >> 1, 1 if f % 2 == 0 else -1
        z, y, x = np.nonzero(geo == b["code"])
        assert z.size > 0
        nb = [z, y, x]
        nb[2 - axis] = nb[2 - axis] + sign  # the fluid neighbour along the face's normal
        assert np.all(geo[tuple(nb)] == 4), FACE_NAMES[f]
        nj, ni = ((nz, ny), (nz, nx), (ny, nx))[axis]
        t = b["table"]
        assert t.shape == (nj, ni) and t.dtype == np.float32 and ni != nj
        jj, ii = ((z, y), (z, x), (y, x))[axis]
        for other in (np.ascontiguousarray(t.T).reshape(t.shape), t[::-1], t[:, ::-1]):
            assert np.count_nonzero(other[jj, ii] != t[jj, ii]) > z.size // 2, FACE_NAMES[f]
    rho, ux, uy, uz = fields
    assert np.all(rho == 1) and all(not np.any(u[(geo == 4) | (geo == 1) | (geo == 0)]) for u in (ux, uy, uz))


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_fields_are_the_oracle_initial_state(oracle, lbm, cfg):
    """The update kernel's equilibrium of box_generic's fields is the oracle's initial state on
    every boundary cell (velocity codes at u_bc with the table value, pressure codes at rest) and
    at rest elsewhere: a lattice initialised from the fields starts where the oracle starts."""
    from lbm_amd import cases
    geo, bcs, (rho, ux, uy, uz) = cases.box_generic(*SHAPES[0], cfg)
    f0 = oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs).f()
    rest = oracle.feq(1.0, 0.0, 0.0, 0.0)
    plain = (geo == 4) | (geo == 1)
    assert np.array_equal(f0[:, plain].view(np.uint32), np.broadcast_to(rest[:, None], f0[:, plain].shape).view(np.uint32))
    for z, y, x in zip(*np.nonzero(geo > 1)):
        if geo[z, y, x] == 4:
            continue
        want = oracle.feq(rho[z, y, x], ux[z, y, x], uy[z, y, x], uz[z, y, x])
        assert np.array_equal(f0[:, z, y, x].view(np.uint32), want.view(np.uint32)), (z, y, x)
    for b in bcs:
        u = [a[geo == b["code"]] for a in (ux, uy, uz)]
        assert all(np.all(a != 0) for a in u) if b["kind"] != 2 else not any(np.any(a) for a in u)


def test_patches_touch(lbm):
    """PX meets NY and NY meets PZ: some fluid cells have NEE neighbours on two faces."""
    from lbm_amd import cases
    geo, bcs, _ = cases.box_generic(*SHAPES[0], 0)
    fl = geo == 4
    faces = np.zeros(geo.shape, np.int32)
    for b in bcs:
        axis, sign = b["face"] >> 1, 1 if b["face"] % 2 == 0 else -1
        e = (Q_EX, Q_EY, Q_EZ)[axis]
        for q in range(1, 19):
            if e[q] == sign:
                faces |= np.where(np.roll(geo == b["code"], (Q_EZ[q], Q_EY[q], Q_EX[q]), (0, 1, 2)) & fl, 1 << b["face"], 0)
    both = lambda a, b: np.count_nonzero((faces & (1 << a) != 0) & (faces & (1 << b) != 0))  # noqa: E731
    assert both(0, 3) > 0 and both(3, 4) > 0


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_stays_finite(oracle, lbm, shape, cfg):
    from lbm_amd import cases
    geo, bcs, _ = cases.box_generic(*shape, cfg)
    o = oracle.Oracle(oracle.GENERIC, geo, 0.6, bcs=bcs)
    o.step(40)
    fl = geo == 4
    assert all(np.all(np.isfinite(a[fl])) for a in o.macros())
    assert np.all(np.isfinite(o.f()[:, fl]))
    assert o.bad_reads() == 0
    assert np.any(o.macros()[1][fl] != 0)


@functools.lru_cache(maxsize=None)
def _base(cfg):
    import orc
    from lbm_amd import cases
    geo, bcs, _ = cases.box_generic(*SHAPES[0], cfg)
    return _macro_bits(orc, geo, bcs, 3)


def _with_table(cfg, face, table):
    from lbm_amd import cases
    geo, bcs, _ = cases.box_generic(*SHAPES[0], cfg)
    bcs[face] = dict(bcs[face], table=np.ascontiguousarray(table, np.float32))
    return geo, bcs


PERTURB = {
    "transposed": lambda t: np.ascontiguousarray(t.T).reshape(t.shape),  # the other raster order
    "flip_j": lambda t: t[::-1],
    "flip_i": lambda t: t[:, ::-1],
}


@pytest.mark.parametrize("how", list(PERTURB))
@pytest.mark.parametrize("kind", [0, 1], ids=["velocity", "velocity_rho"])
@pytest.mark.parametrize("face", range(6), ids=FACE_NAMES)
def test_table_raster_changes_bits(oracle, lbm, face, kind, how):
    """A face's table read in the wrong raster -- transposed, or flipped along either axis --
    changes the oracle's fluid (rho, u) bits after 3 steps, for both velocity kinds."""
    from lbm_amd import cases
    cfg = (kind - face) % 3
    geo, bcs, _ = cases.box_generic(*SHAPES[0], cfg)
    assert bcs[face]["kind"] == kind
    geo, bcs = _with_table(cfg, face, PERTURB[how](bcs[face]["table"]))
    assert np.any(_macro_bits(oracle, geo, bcs, 3) != _base(cfg)), (FACE_NAMES[face], how)


@pytest.mark.parametrize("face", range(6), ids=FACE_NAMES)
def test_pressure_table_is_ignored(oracle, lbm, face):
    """A pressure code takes u of its fluid neighbour: its table, any table, changes nothing."""
    from lbm_amd import cases
    cfg = (2 - face) % 3
    geo, bcs, _ = cases.box_generic(*SHAPES[0], cfg)
    assert bcs[face]["kind"] == 2
    t = bcs[face]["table"]
    for table in (None, t[::-1, ::-1] * np.float32(7)):
        bcs2 = list(bcs)
        bcs2[face] = dict(bcs[face], table=table)
        assert np.array_equal(_macro_bits(oracle, geo, bcs2, 3), _base(cfg)), FACE_NAMES[face]
