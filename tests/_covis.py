"""Two independent restatements of ViGraph::computeCovisibilities (okvis_ceres/src/ViGraph.cpp:727-785)
on an okvisgpu_problem's observation lists. INFRASTRUCTURE ONLY: the checker of
okvisgpu_covisibilities.

A landmark that is not excluded adds 1 to counts[i][j] for every ordered pair i != j of the distinct
poses it is observed from (two cameras of one frame are one pose), makes each of those poses visible
and adds 1 to its n_observed. All integers: the device result is compared with np.array_equal."""
import numpy as np


def _finish(counts, n_observed):
    counts = np.asarray(counts, dtype=np.int32)
    n_observed = np.asarray(n_observed, dtype=np.int32)
    n_pairs = int((np.triu(counts, 1) > 0).sum())
    return {"counts": counts, "n_observed": n_observed, "visible": n_observed > 0, "n_pairs": n_pairs,
            "n_visible": int((n_observed > 0).sum()), "any": n_pairs > 0}


def literal(obs_pose, obs_landmark, n_poses, n_landmarks, excluded=None):
    """As the reference walks it: per landmark the std::set of frames, then the pair loop."""
    frames = [set() for _ in range(n_landmarks)]
    for p, l in zip(obs_pose, obs_landmark):
        frames[int(l)].add(int(p))
    counts = [[0] * n_poses for _ in range(n_poses)]
    n_observed = [0] * n_poses
    for l, fs in enumerate(frames):
        if excluded is not None and excluded[l]:
            continue
        for i in fs:
            n_observed[i] += 1
            for j in fs:
                if i != j:
                    counts[i][j] += 1
    return _finish(counts, n_observed)


def matrix(obs_pose, obs_landmark, n_poses, n_landmarks, excluded=None):
    """The Gram product of the de-duplicated 0/1 visibility matrix."""
    B = np.zeros((n_landmarks, n_poses), dtype=np.int64)
    B[np.asarray(obs_landmark, dtype=np.int64), np.asarray(obs_pose, dtype=np.int64)] = 1
    if excluded is not None:
        B[np.asarray(excluded) != 0] = 0
    G = B.T @ B
    n_observed = np.diag(G).copy()
    np.fill_diagonal(G, 0)
    return _finish(G, n_observed)


def raw_pair_count(obs_pose, obs_landmark, n_poses, n_landmarks):
    """What a count over raw observation pairs gives (no de-duplication of a frame's two cameras):
    the Gram product of the observation-count matrix. Differs from `matrix` on stereo input."""
    B = np.zeros((n_landmarks, n_poses), dtype=np.int64)
    np.add.at(B, (np.asarray(obs_landmark, dtype=np.int64), np.asarray(obs_pose, dtype=np.int64)), 1)
    G = B.T @ B
    np.fill_diagonal(G, 0)
    return G


def of_problem(q, excluded=None, which=matrix):
    """A restatement on an OwnedProblem."""
    return which(q.obs_pose, q.obs_landmark, len(q.poses), len(q.landmarks), excluded)
