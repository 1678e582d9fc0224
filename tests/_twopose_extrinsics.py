"""TwoPoseExtrinsicsGraphError test infrastructure: the calibrating pose-graph edge (D = 6 + 6 C).

  * schur(): the CPU reference of compute(): the edge's reprojection residuals as an okvisgpu_problem
    with every extrinsics block variable (_twopose.SceneProblem), reduced by the oracle without
    scaling or damping. The Schur complement onto [pose 1, camera 0, camera 1, ...] is H00_ and its
    right-hand side is -b0_, provided the reference keyframe is at the origin, no observation has
    |r| > 3 and every landmark has full rank (checked here, so a scene that breaks the premise fails
    loudly instead of comparing different things).
  * decompose(): J_ and DeltaX_ from H00_ / b0_ as TwoPoseExtrinsicsGraphError.cpp:308-318.
  * evaluate(): numpy restatement of EvaluateWithMinimalJacobians (:393-610).
"""
import ctypes as C

import numpy as np

import _twopose as tp
import okvisgpu as og


def qmul(a, b):
    """Hamilton product, coefficients (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def qinv(q):
    return np.array([-q[0], -q[1], -q[2], q[3]]) / np.dot(q, q)


def qnorm(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def plus(q):
    """okvis::kinematics::plus (operators.hpp:64-76)."""
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def oplus(q):
    """okvis::kinematics::oplus (operators.hpp:78-90)."""
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def cross(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def relative_pose(T0, T1):
    """T_S0S1 = T_WS0^-1 T_WS1 as [r, q xyzw]."""
    q0, q1 = qnorm(T0[3:]), qnorm(T1[3:])
    return np.r_[tp.rot(q0).T @ (T1[:3] - T0[:3]), qnorm(qmul(qinv(q0), q1))]


def schur(oracle, edge, cams, ex):
    """(H00_, b0_) of the edge from the oracle's reduced system; asserts the premises above."""
    assert np.array_equal(edge["ref_pose"], [0, 0, 0, 0, 0, 0, 1])
    sp = tp.SceneProblem(edge, cams, ex)
    sp.xc = np.zeros(len(cams), dtype=np.uint8)
    sp.problem.extrinsics_constant = sp.xc.ctypes.data_as(C.POINTER(C.c_uint8))
    r, _, _ = oracle.eval_reprojection(sp.ptr(), len(sp.op))
    assert np.linalg.norm(r, axis=1).max() < 3.0, "scene has an outlier: the Schur reference does not apply"
    for obs in edge["observations"]:
        assert len(obs) >= 2, "scene has a rank-deficient landmark: the Schur reference does not apply"
    S, rhs, _, rc = oracle.linearize_reduce(sp.ptr(), False, 0.0)
    D = 6 + 6 * len(cams)
    assert rc == 0 and S.shape == (D, D)
    return S, -rhs


def kept(lam, D):
    return lam > 1e-8 * D * lam.max()


def decompose(H, b0):
    """J_ = D^(1/2) E^T (ascending, zero rows for dropped eigenvalues), DeltaX_ = -E D^-1 E^T b0_."""
    D = len(b0)
    lam, E = np.linalg.eigh(H)
    k = kept(lam, D)
    J = np.where(k, np.sqrt(np.where(k, lam, 0.0)), 0.0)[:, None] * E.T
    M = E * np.where(k, 1.0 / np.sqrt(np.where(k, lam, 1.0)), 0.0)[None, :]
    return J, -M @ (M.T @ b0)


def evaluate(ref_pose, other_pose, ex, delta_x, J, lin_point, lin_ex, seen):
    """r [D], J_ref [D,6], J_other [D,6], J_extrinsics [C,D,6] (minimal) of one edge."""
    nc = len(ex)
    D = 6 + 6 * nc
    T0, T1 = np.asarray(ref_pose, dtype=np.float64), np.asarray(other_pose, dtype=np.float64)
    q0, q1, ql = qnorm(T0[3:]), qnorm(T1[3:]), qnorm(lin_point[3:])
    C_S0W = tp.rot(q0).T
    rel = relative_pose(T0, T1)
    d = np.zeros(D)
    d[:3] = rel[:3] - lin_point[:3]
    d[3:6] = 2.0 * qmul(rel[3:], qinv(ql))[:3]
    Jx = np.zeros((nc, D, 6))
    for c in range(nc):
        if not seen[c]:
            continue
        dq = qmul(qnorm(ex[c][3:]), qinv(qnorm(lin_ex[c][3:])))
        d[6 + 6 * c:9 + 6 * c] = ex[c][:3] - lin_ex[c][:3]
        d[9 + 6 * c:12 + 6 * c] = 2.0 * dq[:3]
        Jerrex = np.zeros((6, 6))
        Jerrex[:3, :3] = np.eye(3)
        Jerrex[3:, 3:] = oplus(dq)[:3, :3]
        Jx[c] = J[:, 6 + 6 * c:12 + 6 * c] @ Jerrex
    r = J @ (delta_x + d)
    B = (plus(qinv(q0)) @ oplus(qmul(q1, qinv(ql))))[:3, :3]
    Jerr = np.zeros((6, 6))
    Jerr[:3, :3] = C_S0W
    Jerr[3:, 3:] = B
    JerrRef = np.zeros((6, 6))
    JerrRef[:3, :3] = -C_S0W
    JerrRef[:3, 3:] = C_S0W @ cross(T1[:3] - T0[:3])
    JerrRef[3:, 3:] = -B
    return r, J[:, :6] @ JerrRef, J[:, :6] @ Jerr, Jx


def pose_plus(oracle, x, delta):
    out = np.zeros(7)
    oracle.lib().oracle_pose_plus(og.dptr(np.ascontiguousarray(x, dtype=np.float64)),
                                  og.dptr(np.ascontiguousarray(delta, dtype=np.float64)), og.dptr(out))
    return out


def perturbed(oracle, poses, rng, sigma_r, sigma_a):
    """Each [7] pose moved by a random minimal step of the given sizes (m, rad)."""
    return np.array([pose_plus(oracle, p, np.r_[rng.normal(0, sigma_r, 3), rng.normal(0, sigma_a, 3)]) for p in poses])


def drop_observations(edge, pred):
    """A copy of the edge without the observations pred(landmark index, observation) selects."""
    obs = [[o for o in lo if not pred(l, o)] for l, lo in enumerate(edge["observations"])]
    return {**edge, "observations": obs}
