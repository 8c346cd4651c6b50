"""The relaxation time across its range, bit for bit against the CPU oracle.

tau feeds the fast quotient (its reciprocal and correction), omc = 1.0f - 1.0f / tau of every NEE
value (the static NEE records and k_nee_fix included), verify_fast_div's range gate
(0.0625 <= tau <= 16, else the compiler's division) and the stress read-out's k = 1 - 0.5 / tau
(tests/test_gpu_stress.py::test_stress_tau).  The values: 0.5 (omc = -1, zero viscosity), 0.51, 0.75,
1.0 (omc = 0: the NEE value is the boundary equilibrium), 2.0, 16.0 (the gate's last fast value) and
17.0 (the exact division without LBM_TUNE_EXACT_DIV).  The oracle stays finite for 40 steps on
every lattice below at each of them, and at 40.0."""
import pytest

from test_gpu_parity import assert_bitwise, assert_residuals, fp64_sum

pytestmark = pytest.mark.gpu

TAUS = [0.5, 0.51, 0.75, 1.0, 2.0, 16.0, 17.0]


def _make(oracle, case, tau):
    """(lattice, oracle, geo, assert_bitwise's kind) of a case at tau."""
    from lbm_amd import cases
    if case == "ldc":
        lat, geo = cases.ldc(13, 11, 7, tau=tau)
        return lat, oracle.Oracle(oracle.LDC, geo, tau, ldc_order=oracle.TWO_PHASE), geo, 0
    if case == "poiseuille":
        lat, geo = cases.poiseuille(13, 24, 11, tau=tau)
        return lat, oracle.Oracle(oracle.POISEUILLE, geo, tau), geo, 1
    geo, bcs, fields = cases.duct_generic(24, 14, 12)
    return cases.generic(geo, bcs, fields, tau=tau), oracle.Oracle(oracle.GENERIC, geo, tau, bcs=bcs), geo, 2


@pytest.mark.parametrize("case", ["ldc", "poiseuille", "duct"])
@pytest.mark.parametrize("tau", TAUS)
def test_tau_sweep_bitwise(gpu, oracle, tau, case, cells_per_lane, row_axis):
    lat, o, geo, kind = _make(oracle, case, tau)
    fp64_sum(o)
    assert lat.numerics()["fast_div"] == (0.0625 <= tau <= 16.0)
    for s in (1, 1, 20):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, kind, f"{case} tau {tau} +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0
    lat.close()


# LBM_TUNE_NEE_FIX -> the path the pipe takes.  Measured on an MI355X: with LBM_TUNE_NEE_FIX 2 the
# 300-cell rows of (17, 300, 21) do not take NEE records but k_nee_fix -- {'path': 'fix',
# 'max_records': 0}, also with LBM_TUNE_GROUPS 1 and LBM_TUNE_GRID_STRIDE 1: 256-cell chunks do not
# tile rows of 300 cells, so its sparse chunk list has partly idle chunks and carries lane masks,
# which the records kernel does not take (lbm_ctx.hip build_range, launch_step).  (20, 512, 18),
# whose rows are two whole chunks, takes records ({'path': 'records', 'max_records': 1}), so that
# shape carries the records cases.
NEE_PIPES = [((17, 300, 21), 1, "blocks"), ((17, 300, 21), 3, "fix"), ((17, 300, 21), 2, "fix"),
             ((20, 512, 18), 2, "records")]


@pytest.mark.parametrize("shape,nee_fix,path", NEE_PIPES,
                         ids=["300-nee_blocks", "300-nee_fix", "300-nee_records_knob", "512-nee_records"])
@pytest.mark.parametrize("tau", [0.51, 1.0, 17.0])
def test_tau_nee_paths_bitwise(gpu, oracle, knob, tau, shape, nee_fix, path):
    """omc in the NEE blocks, k_nee_fix and the NEE records (static part computed at lbm_create),
    on pipes whose chunk waves collide the NEE-adjacent cells."""
    from lbm_amd import cases
    import lbm_amd
    knob(lbm_amd.TUNE_CELLS_PER_LANE, 4)
    knob(lbm_amd.TUNE_NEE_FIX, nee_fix)
    lat, geo = cases.poiseuille(*shape, tau=tau)
    assert lat.layout()["row_axis"] == 2
    assert lat.nee_path()["path"] == path, lat.nee_path()
    o = fp64_sum(oracle.Oracle(oracle.POISEUILLE, geo, tau))
    for s in (1, 2, 20):
        hg, ho = lat.step(s), o.step(s)
        assert_bitwise(lat, o, geo, 1, f"pipe tau {tau} +{s}")
        assert_residuals(hg, ho)
    assert o.bad_reads() == 0
    lat.close()


def test_tau_large_exact_path(gpu, oracle):
    """tau = 40 lies outside the fast quotient's verified range: the context takes the compiler's
    division on its own, no knob set."""
    from lbm_amd import cases
    lat, geo = cases.ldc(24, tau=40.0)
    assert not lat.numerics()["fast_div"]
    o = oracle.Oracle(oracle.LDC, geo, 40.0, ldc_order=oracle.TWO_PHASE)
    lat.step(30)
    o.step(30)
    assert_bitwise(lat, o, geo, 0, "ldc24 tau 40")
    lat.close()
