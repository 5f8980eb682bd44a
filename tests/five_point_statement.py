"""An independent float64 statement of the five-point essential-matrix solver, and the synthetic scenes the five-point
tests share.  It restates nister-stewenius/src/lib.rs:50-280 with numpy's LAPACK (eigh, solve, eig; eig's eigenvectors are polished by
inverse iteration, see inverse_iteration) and shares no code
with include/akz_five_point_math.h.

One deliberate difference from the reference: lib.rs:230 takes rows 5..8 of the action matrix's eigenvector; the
coordinates (x, y, z, 1) are its rows 6..9 (monomial order xx xy yy xz yz zz x y z 1, and the -1 rows of lib.rs:274-277).
`rows=(5, 9)` evaluates the reference as written."""
import numpy as np

EIGEN_THRESHOLD = 1e-12
XXX, XXY, XYY, YYY, XXZ, XYZ, YYZ, XZZ, YZZ, ZZZ, XX, XY, YY, XZ, YZ, ZZ, X, Y, Z, ONE = range(20)


def epipolar_matrix(a, b):
    """lib.rs:50-66: row i = kron(a_i, b_i), entry 3 j + k = a[j] b[k]."""
    return np.stack([np.kron(a[i], b[i]) for i in range(5)])


def nullspace_basis(a, b):
    """lib.rs:68-96: the eigenvectors of the four smallest eigenvalues of A^T A, or None unless exactly four are <= 1e-12."""
    m = epipolar_matrix(a, b)
    if not np.all(np.isfinite(m)):
        return None
    val, vec = np.linalg.eigh(m.T @ m)
    if int(np.sum(val <= EIGEN_THRESHOLD)) != 4:
        return None
    return vec[:, :4]


def o1(a, b):
    r = np.zeros(20)
    r[XX] = a[0] * b[0]
    r[XY] = a[0] * b[1] + a[1] * b[0]
    r[XZ] = a[0] * b[2] + a[2] * b[0]
    r[YY] = a[1] * b[1]
    r[YZ] = a[1] * b[2] + a[2] * b[1]
    r[ZZ] = a[2] * b[2]
    r[X] = a[0] * b[3] + a[3] * b[0]
    r[Y] = a[1] * b[3] + a[3] * b[1]
    r[Z] = a[2] * b[3] + a[3] * b[2]
    r[ONE] = a[3] * b[3]
    return r


def o2(a, b):
    r = np.zeros(20)
    r[XXX] = a[XX] * b[0]
    r[XXY] = a[XX] * b[1] + a[XY] * b[0]
    r[XXZ] = a[XX] * b[2] + a[XZ] * b[0]
    r[XYY] = a[XY] * b[1] + a[YY] * b[0]
    r[XYZ] = a[XY] * b[2] + a[YZ] * b[0] + a[XZ] * b[1]
    r[XZZ] = a[XZ] * b[2] + a[ZZ] * b[0]
    r[YYY] = a[YY] * b[1]
    r[YYZ] = a[YY] * b[2] + a[YZ] * b[1]
    r[YZZ] = a[YZ] * b[2] + a[ZZ] * b[1]
    r[ZZZ] = a[ZZ] * b[2]
    r[XX] = a[XX] * b[3] + a[X] * b[0]
    r[XY] = a[XY] * b[3] + a[X] * b[1] + a[Y] * b[0]
    r[XZ] = a[XZ] * b[3] + a[X] * b[2] + a[Z] * b[0]
    r[YY] = a[YY] * b[3] + a[Y] * b[1]
    r[YZ] = a[YZ] * b[3] + a[Y] * b[2] + a[Z] * b[1]
    r[ZZ] = a[ZZ] * b[3] + a[Z] * b[2]
    r[X] = a[X] * b[3] + a[ONE] * b[0]
    r[Y] = a[Y] * b[3] + a[ONE] * b[1]
    r[Z] = a[Z] * b[3] + a[ONE] * b[2]
    r[ONE] = a[ONE] * b[3]
    return r


def constraints(basis):
    """lib.rs:138-204: the 10 x 20 constraint matrix."""
    e = basis.reshape(3, 3, 4)
    m = np.zeros((10, 20))
    m[0] = (o2(o1(e[0][1], e[1][2]) - o1(e[0][2], e[1][1]), e[2][0])
            + o2(o1(e[0][2], e[1][0]) - o1(e[0][0], e[1][2]), e[2][1])
            + o2(o1(e[0][0], e[1][1]) - o1(e[0][1], e[1][0]), e[2][2]))
    eet = [[o1(e[i][0], e[j][0]) + o1(e[i][1], e[j][1]) + o1(e[i][2], e[j][2]) for j in range(3)] for i in range(3)]
    trace = 0.5 * (eet[0][0] + eet[1][1] + eet[2][2])
    ell = [[eet[i][j] - (trace if i == j else 0.0) for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(3):
            m[1 + 3 * i + j] = o2(ell[i][0], e[0][j]) + o2(ell[i][1], e[1][j]) + o2(ell[i][2], e[2][j])
    return m


def action_matrix(c):
    """lib.rs:256-277."""
    m = np.linalg.solve(c[:, :10], c[:, 10:])
    at = np.zeros((10, 10))
    at[:3] = m[:3]
    at[3], at[4], at[5] = m[4], m[5], m[7]
    at[6, 0] = at[7, 1] = at[8, 3] = at[9, 6] = -1.0
    return at


def inverse_iteration(at, lam, v, steps=2):
    """eig's eigenvector polished with numpy.linalg.solve.  The action matrix's eigenvalues can span six orders of
    magnitude (a solution whose last coordinate nearly vanishes in LAPACK's basis of the null space); eig's vectors are then
    accurate to eps * |At| / gap only — 2.9e-6 in E on scene 488 of the seeded set, cubic residual 1.3e-7.  Two steps of
    inverse iteration at eig's own eigenvalue bring that to 5e-9 and 2e-10."""
    for _ in range(steps):
        try:
            y = np.linalg.solve(at - lam * np.eye(len(at)), v)
        except np.linalg.LinAlgError:
            break
        n = np.linalg.norm(y)
        if not np.isfinite(n) or n == 0.0:
            break
        v = y / n
    return v


def essentials(a, b, rows=(6, 10), with_eigenvalues=False):
    """All solutions for five matches (unit bearings a, b: [5, 3]) in ascending order of eigenvalue: [n, 3, 3] with
    b^T E a = 0, each as basis * v[rows] laid out column-major (Matrix3::from_iterator)."""
    empty = (np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0, complex)) if with_eigenvalues else np.zeros((0, 3, 3))
    basis = nullspace_basis(np.asarray(a, float), np.asarray(b, float))
    if basis is None:
        return empty
    c = constraints(basis)
    try:
        at = action_matrix(c)
    except np.linalg.LinAlgError:
        return empty
    val, vec = np.linalg.eig(at)
    real = np.flatnonzero(val.imag == 0)
    real = real[np.argsort(val.real[real], kind="stable")]
    out = []
    for i in real:
        v = inverse_iteration(at, val[i].real, vec[:, i].real)
        e = (basis @ v[rows[0]:rows[1]]).reshape(3, 3).T
        if np.all(np.isfinite(e)):
            out.append(e)
    es = np.array(out).reshape(-1, 3, 3)
    return (es, val.real[real], val) if with_eigenvalues else es


def knife_edge(all_eigenvalues):
    """A scene whose eigenvalues (all ten, complex) have a minimum pairwise gap below 1e-3 relative to max(1, |lambda|): a
    nearly double root or a nearly real pair, where the number of real solutions is legitimately unstable."""
    v = np.asarray(all_eigenvalues)
    for i in range(len(v)):
        for j in range(i + 1, len(v)):
            if abs(v[i] - v[j]) < 1e-3 * max(1.0, abs(v[i]), abs(v[j])):
                return True
    return False


# ---- scenes ----
def rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def scene(rng, n=5):
    """(a [n, 3], b [n, 3], R, t, E): rotation angle uniform in 0.02-0.3 rad about a random axis, |t| in 0.2-1, points in
    x +-2, y +-1.5, z 3-9, unit bearings; b = R p + t, E = [t]x R so that b^T E a = 0."""
    r = rotation(rng.normal(size=3), rng.uniform(0.02, 0.3))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * rng.uniform(0.2, 1.0)
    p = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], axis=1)
    q = p @ r.T + t
    a = p / np.linalg.norm(p, axis=1, keepdims=True)
    b = q / np.linalg.norm(q, axis=1, keepdims=True)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return a, b, r, t, tx @ r


SEED = 0x5EED5


def scenes(count=512, seed=SEED):
    rng = np.random.default_rng(seed)
    return [scene(rng) for _ in range(count)]


def normalised(e):
    e = np.asarray(e, float)
    return e / np.linalg.norm(e)


def distance(e0, e1):
    """Frobenius distance of two essential matrices, both normalised, up to sign."""
    e0, e1 = normalised(e0), normalised(e1)
    return min(np.linalg.norm(e0 - e1), np.linalg.norm(e0 + e1))


def cubic_residual(e):
    e = normalised(e)
    return np.abs(2 * e @ e.T @ e - np.trace(e @ e.T) * e).max()
