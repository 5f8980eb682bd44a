"""include/akz_five_point_math.h built by the host compiler (tests/five_point_checker.py) against the independent float64
statement of tests/five_point_statement.py, on 512 seeded exact scenes.  No GPU.

Counterparts.  Both sides emit their solutions in ascending order of the action matrix's eigenvalue, but that eigenvalue is
-x / w in the coordinates of the null-space basis, and the basis of a four-fold eigenvalue is not pinned (LAPACK's and the
Jacobi iteration's differ by a rotation): the order is comparable between device and host build (same header), not between
host build and statement.  A solution's counterpart is its nearest neighbour, and the matching must be one-to-one.

Measured on this machine (seed 0x5EED5, 512 scenes; print_measurements() prints them on every run):
  knife-edge scenes                              7 of 512 (1.4 %)
  solution counts 2 / 4 / 6 / 8                  37 / 241 / 233 / 1
  worst host-build-vs-statement distance         5.2e-9    -> asserted at 5.2e-8 (<= 1e-6)
  the same on the knife-edge scenes' common ones 3.3e-8    -> asserted at 3.3e-7 (<= 1e-6)
  worst distance of the true E, host build       2.3e-10   (statement: 7.3e-10)
  worst |b^T E a| (E normalised)                 3.6e-14   -> asserted at 3.6e-13
  worst |det E|                                  3.8e-11   -> asserted at 3.8e-10
  worst |2 E E^T E - tr(E E^T) E|                3.1e-10   -> asserted at 3.1e-9
"""
import numpy as np
import pytest

import five_point_checker as ck
import five_point_statement as st

TOL_E = 5.2e-8          # 10 x the measured worst deviation; the issue's cap is 1e-6
TOL_E_KNIFE = 3.3e-7    # the same on the knife-edge scenes' common solutions (conditioning grows with 1 / gap there)
TOL_EPIPOLAR = 3.6e-13
TOL_DET = 3.8e-10
TOL_CUBIC = 3.1e-9
assert TOL_E <= 1e-6 and TOL_E_KNIFE <= 1e-6


@pytest.fixture(scope="module")
def solved():
    """per scene: (a, b, E_true, statement solutions, all ten statement eigenvalues, host solutions)"""
    out = []
    for a, b, _, _, e_true in st.scenes():
        es, _, all_values = st.essentials(a, b, with_eigenvalues=True)
        out.append((a, b, e_true, es, all_values, ck.solve(a, b)))
    return out


def match(es, eh):
    """nearest host solution of every statement solution -> (indices, distances)"""
    d = np.array([[st.distance(e0, e1) for e1 in eh] for e0 in es]).reshape(len(es), len(eh))
    nn = d.argmin(axis=1)
    return nn, d[np.arange(len(es)), nn]


def test_print_measurements(solved):
    knife = sum(st.knife_edge(v) for *_, v, _ in solved)
    worst = max((match(es, eh)[1].max() for _, _, _, es, v, eh in solved if not st.knife_edge(v) and len(es) and len(eh)), default=0.0)
    truth = max(min(st.distance(e, x) for x in eh) for _, _, e, _, v, eh in solved if not st.knife_edge(v))
    hist = np.bincount([len(eh) for *_, eh in solved], minlength=11)
    print(f"\nknife-edge {knife} of {len(solved)}; worst deviation {worst:.3e}; worst distance of the true E {truth:.3e}; "
          f"solution counts {dict((k, int(n)) for k, n in enumerate(hist) if n)}")


def test_knife_edge_scenes_are_few(solved):
    knife = sum(st.knife_edge(v) for *_, v, _ in solved)
    assert knife <= 0.05 * len(solved), knife


def test_host_build_matches_the_statement(solved):
    for i, (_, _, e_true, es, values, eh) in enumerate(solved):
        if st.knife_edge(values):
            # a nearly double root or a nearly real pair: the solutions both sides have = the mutual nearest neighbours
            if len(es) and len(eh):
                nn, d = match(es, eh)
                back, _ = match(eh, es)
                common = [k for k in range(len(es)) if back[nn[k]] == k]
                assert common, i
                assert max(d[k] for k in common) < TOL_E_KNIFE, (i, d)
            continue
        assert len(es) == len(eh), (i, len(es), len(eh))
        nn, d = match(es, eh)
        assert len(set(nn.tolist())) == len(nn), (i, nn)
        assert d.max() < TOL_E, (i, d)
        assert min(st.distance(e_true, x) for x in eh) < TOL_E, i


def test_every_solution_is_an_essential_matrix(solved):
    for i, (a, b, _, _, _, eh) in enumerate(solved):
        assert len(eh) > 0, i
        for e in eh:
            n = st.normalised(e)
            assert np.abs(np.einsum("ni,ij,nj->n", b, n, a)).max() < TOL_EPIPOLAR, i
            assert abs(np.linalg.det(n)) < TOL_DET, i
            assert st.cubic_residual(e) < TOL_CUBIC, i


def test_unused_slots_are_untouched():
    a, b, *_ = st.scenes(4)[3]
    E, n = ck.essentials(a, b, np.arange(5)[None], fill=7.0)
    assert 0 < n[0] <= 10
    assert np.all(E[0, n[0]:] == 7.0)
    assert np.all(np.isfinite(E[0, :n[0]]))


def test_rejected_inputs_give_no_solution():
    a, b, *_ = st.scenes(1)[0]
    # a repeated match: the epipolar matrix has rank 4, nullity 5
    E, n = ck.essentials(a, b, np.array([[0, 1, 2, 3, 3]]))
    assert n[0] == 0
    bad = a.copy()
    bad[2, 1] = np.nan
    E, n = ck.essentials(bad, b, np.arange(5)[None])
    assert n[0] == 0
    assert len(st.essentials(a[[0, 1, 2, 3, 3]], b[[0, 1, 2, 3, 3]])) == 0
    assert len(st.essentials(bad, b)) == 0


def test_the_reference_rows_do_not_solve_the_problem():
    """lib.rs:230 as written (rows 5..8): the true E is not among the solutions; rows 6..9: it is."""
    hits_ref = hits = 0
    for a, b, _, _, e_true in st.scenes(64):
        ref = st.essentials(a, b, rows=(5, 9))
        ours = st.essentials(a, b)
        hits_ref += bool(len(ref)) and min(st.distance(e_true, x) for x in ref) < 1e-6
        hits += min(st.distance(e_true, x) for x in ours) < 1e-6
    assert hits == 64 and hits_ref == 0


# ---- the polynomial products on the reference's own two unit-test vectors (lib.rs:368-417) ----
def evaluate(p, x, y, z):
    mono = [x * x * x, x * x * y, x * y * y, y * y * y, x * x * z, x * y * z, y * y * z, x * z * z, y * z * z, z * z * z,
            x * x, x * y, y * y, x * z, y * z, z * z, x, y, z, 1.0]
    return float(np.dot(p, mono))


def linear(v):
    p = np.zeros(20)
    p[16:20] = v
    return p


GRID = [(float(x), float(y), float(z)) for z in range(-5, 5) for y in range(-5, 5) for x in range(-5, 5)]


def test_o1_is_polynomial_multiplication():
    p1, p2 = np.array([0.1, 0.8, 0.3, 0.2]), np.array([0.5, 0.45, 0.82, 0.15])
    for fn in (ck.o1, st.o1):
        p3 = fn(p1, p2)
        for x, y, z in GRID:
            assert abs(evaluate(p3, x, y, z) - evaluate(linear(p1), x, y, z) * evaluate(linear(p2), x, y, z)) < 1e-6


def test_o2_is_polynomial_multiplication():
    p1 = np.zeros(20)
    p1[10:20] = [0.2, 0.81, 0.91, 0.66, 0.88, 0.14, 0.97, 0.3, 0.38, 0.72]   # xx xy yy xz yz zz x y z 1
    p2 = np.array([0.5, 0.45, 0.82, 0.15])
    for fn in (ck.o2, st.o2):
        p3 = fn(p1, p2)
        for x, y, z in GRID:
            assert abs(evaluate(p3, x, y, z) - evaluate(p1, x, y, z) * evaluate(linear(p2), x, y, z)) < 1e-8
