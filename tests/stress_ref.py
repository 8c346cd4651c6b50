"""Plain numpy restatement of lbm_get_stress / lbm_get_shear (include/lbm.h), the checker of
tests/test_stress_ref.py and tests/test_gpu_stress.py.

Input: f_src, the populations one step earlier ([19][nz][ny][nx], e.g. oracle.Oracle.f() after
k - 1 steps), the reference codes geo and tau.  The last step pulled

    pulled[q](x) = f_src[opp q](x)   where geo(x - e_q) == 1   (half-way bounce-back)
                 = f_src[q](x - e_q) otherwise                 (NEE slots and fluid alike)

(the very first step of every case but LDC pulls the wall slots as they are, like the reference:
pull's raw_walls), and the stress is the fixed fp64 arithmetic of include/lbm.h on those 19 fp32 values, left to
right.  Shifts wrap around the box: no fluid cell of the tested geometries lies on a box face
(the uniform-shear box is uniform, so the wrap is the identity there).
"""
import numpy as np

# e_q as k_moments' momentum sums imply: q1..6 = +-x, +-y, +-z; 7..10 xy; 11..14 xz; 15..18 yz
EX = (0, 1, -1, 0, 0, 0, 0, 1, 1, -1, -1, 1, 1, -1, -1, 0, 0, 0, 0)
EY = (0, 0, 0, 1, -1, 0, 0, 1, -1, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1)
EZ = (0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1, 1, 1, -1, -1)
OPP = (0, 2, 1, 4, 3, 6, 5, 10, 9, 8, 7, 14, 13, 12, 11, 18, 17, 16, 15)
W = (1 / 3,) + (1 / 18,) * 6 + (1 / 36,) * 12
COMPONENTS = ("xx", "yy", "zz", "xy", "xz", "yz")


def _from(a, q):
    """a(x - e_q) at every x (arrays are [z][y][x])."""
    return np.roll(a, (EZ[q], EY[q], EX[q]), axis=(0, 1, 2))


def pull(f_src, geo, raw_walls=False):
    """The 19 populations every cell pulled, float32 [19][nz][ny][nx].  raw_walls: the step was
    the first one of a case whose walls do not bounce back at step 0 (every case but LDC: the
    reference's first update reads the wall cells' initial populations as they are), so wall
    slots are pulled like any other; they differ from the bounce-back values only where the
    initial velocity next to a wall is not zero (the inlet rows of a pipe)."""
    f_src = np.asarray(f_src, np.float32)
    wall = np.asarray(geo) == 1
    out = np.empty_like(f_src)
    out[0] = f_src[0]
    for q in range(1, 19):
        out[q] = _from(f_src[q], q)
        if not raw_walls:
            out[q] = np.where(_from(wall, q), f_src[OPP[q]], out[q])
    return out


def wall_adjacent(geo):
    """Cells with a code-1 wall cell among their 18 neighbours x - e_q."""
    wall = np.asarray(geo) == 1
    adj = np.zeros(wall.shape, bool)
    for q in range(1, 19):
        adj |= _from(wall, q)
    return adj


def macros32(p):
    """k_moments' fp32 (rho, ux, uy, uz) of pulled populations p."""
    f = [p[q] for q in range(19)]
    r = np.zeros_like(f[0])
    for q in range(19):
        r = r + f[q]
    with np.errstate(all="ignore"):
        ux = (f[1] - f[2] + f[7] + f[8] - f[9] - f[10] + f[11] + f[12] - f[13] - f[14]) / r
        uy = (f[3] - f[4] + f[7] - f[8] + f[9] - f[10] + f[15] - f[16] + f[17] - f[18]) / r
        uz = (f[5] - f[6] + f[11] - f[12] + f[13] - f[14] + f[15] + f[16] - f[17] - f[18]) / r
    return r, ux, uy, uz


def moments64(p, tau):
    """include/lbm.h's arithmetic in float64: (S [6] in COMPONENTS order, shear), unrounded."""
    d = [p[q].astype(np.float64) for q in range(19)]
    r = d[0]
    for q in range(1, 19):
        r = r + d[q]
    mx = d[1] - d[2] + d[7] + d[8] - d[9] - d[10] + d[11] + d[12] - d[13] - d[14]
    my = d[3] - d[4] + d[7] - d[8] + d[9] - d[10] + d[15] - d[16] + d[17] - d[18]
    mz = d[5] - d[6] + d[11] - d[12] + d[13] - d[14] + d[15] + d[16] - d[17] - d[18]
    pxx = d[1] + d[2] + d[7] + d[8] + d[9] + d[10] + d[11] + d[12] + d[13] + d[14]
    pyy = d[3] + d[4] + d[7] + d[8] + d[9] + d[10] + d[15] + d[16] + d[17] + d[18]
    pzz = d[5] + d[6] + d[11] + d[12] + d[13] + d[14] + d[15] + d[16] + d[17] + d[18]
    pxy = d[7] - d[8] - d[9] + d[10]
    pxz = d[11] - d[12] - d[13] + d[14]
    pyz = d[15] - d[16] - d[17] + d[18]
    c = r / 3.0
    k = 1.0 - 0.5 / np.float64(np.float32(tau))
    with np.errstate(all="ignore"):
        sxx = (-k) * ((pxx - c) - (mx * mx) / r)
        syy = (-k) * ((pyy - c) - (my * my) / r)
        szz = (-k) * ((pzz - c) - (mz * mz) / r)
        sxy = (-k) * (pxy - (mx * my) / r)
        sxz = (-k) * (pxz - (mx * mz) / r)
        syz = (-k) * (pyz - (my * mz) / r)
        pr = ((sxx + syy) + szz) / 3.0
        dxx, dyy, dzz = sxx - pr, syy - pr, szz - pr
        j = 0.5 * ((dxx * dxx + dyy * dyy) + dzz * dzz) + ((sxy * sxy + sxz * sxz) + syz * syz)
        shear = np.sqrt(j)
    return np.stack([sxx, syy, szz, sxy, sxz, syz]), shear


def stress_ref(f_src, geo, tau, fluid, raw_walls=False):
    """What lbm_get_stress / lbm_get_shear return for the step that ran from f_src: a dict with
    stress float32 [6][nz][ny][nx], shear and shear_wall float32 [nz][ny][nx] (exact zeros off-fluid
    / off the wall-adjacent cells), the fluid and wall-adjacent fluid masks, and n_fluid / n_wall.
    raw_walls: see pull (True for step 1 of every case but LDC)."""
    geo = np.asarray(geo)
    fl = geo == fluid
    s64, sh64 = moments64(pull(f_src, geo, raw_walls), tau)
    s = np.where(fl, s64, 0.0).astype(np.float32)
    sh = np.where(fl, sh64, 0.0).astype(np.float32)
    wa = fl & wall_adjacent(geo)
    return {"stress": s, "shear": sh, "shear_wall": np.where(wa, sh, np.float32(0)), "fluid": fl, "wall": wa,
            "n_fluid": int(fl.sum()), "n_wall": int(wa.sum())}


def feq64(rho, u):
    """Second-order equilibrium in float64 (no reference rounding order: the identity test's input)."""
    out = []
    usq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    for q in range(19):
        eu = EX[q] * u[0] + EY[q] * u[1] + EZ[q] * u[2]
        out.append(W[q] * rho * (1.0 + 3.0 * eu + 4.5 * eu * eu - 1.5 * usq))
    return np.array(out)


def uniform_shear_populations(rho, u, S, tau):
    """f_q = feq_q(rho, u) - 3 tau rho w_q (e_q e_q - delta/3) : S, the Chapman-Enskog populations of a
    uniform strain rate S (symmetric 3x3), in float64."""
    S = np.asarray(S, np.float64)
    f = feq64(rho, u)
    for q in range(19):
        e = np.array([EX[q], EY[q], EZ[q]], np.float64)
        qq = np.outer(e, e) - np.eye(3) / 3.0
        f[q] -= 3.0 * tau * rho * W[q] * float(np.sum(qq * S))
    return f
